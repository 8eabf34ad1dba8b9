"""pbrhip -- thin ctypes binding of libgpu_hip.so (the GPU_* / GPUX_* / PBR_* / pbrk_* C ABI).

Used by tests/, bench.py and __graft_entry__.py.  There is no CPU fallback: importing is free, but
`lib()` raises if the HIP library has not been built, and every GPU call needs a real device.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(os.path.dirname(_PKG))                 # vulkan-pbr-renderer_amd/
REPO_ROOT = os.path.dirname(PKG_ROOT)
LIB_PATH = os.path.join(PKG_ROOT, "libgpu_hip.so")

# ---- enums (include/gpu_hip.h) ----
(Format_Invalid, Format_R8UN, Format_RG8UN, Format_RGBA8UN, Format_BGRA8UN, Format_R16F, Format_RG16F, Format_RGB16F,
 Format_RGBA16F, Format_R32F, Format_RG32F, Format_RGB32F, Format_RGBA32F, Format_R8I, Format_R16I, Format_RG16I,
 Format_RGBA16I, Format_R32I, Format_RG32I, Format_RGB32I, Format_RGBA32I, Format_R64I, Format_D16UN,
 Format_D32F_Or_X8D24UN) = range(24)
Format_BC1_RGB_UN, Format_BC1_RGBA_UN, Format_BC3_RGBA_UN, Format_BC5_UN = 26, 27, 28, 29
BC_BLOCK_BYTES = {Format_BC1_RGB_UN: 8, Format_BC1_RGBA_UN: 8, Format_BC3_RGBA_UN: 16, Format_BC5_UN: 16}
PBRK_BC1_RGB, PBRK_BC1_RGBA, PBRK_BC3, PBRK_BC5 = 0, 1, 2, 3
PBR_DDS_FILE_MIPS = 1
PBR_DDS_MAX_LEVELS = 16
PBR_DDS_OUT_SAME, PBR_DDS_OUT_RGBA16F, PBR_DDS_OUT_BC6H_UF16, PBR_DDS_OUT_BC6H_UF16_2R = 0, 1, 2, 3
GPUX_BC6H_OneRegion, GPUX_BC6H_TwoRegions = 0, 1
TextureFlag_StorageImage, TextureFlag_RenderTarget, TextureFlag_HasMipmaps, TextureFlag_Cubemap = 1, 2, 4, 8
BufferFlag_CPU, BufferFlag_GPU, BufferFlag_StorageBuffer = 1, 2, 4
Shade_IBL, Shade_LightShafts = 1, 2
Unit_Prefilter, Unit_Irradiance, Unit_BrdfLut = 0, 1, 2


class GPU_Texture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("depth", C.c_uint32), ("layer_count", C.c_uint32),
                ("mip_level_count", C.c_uint32), ("format", C.c_int), ("flags", C.c_int)]


class GPU_Buffer(C.Structure):
    _fields_ = [("flags", C.c_int), ("size", C.c_uint32), ("data", C.c_void_p)]


class GPU_String(C.Structure):
    _fields_ = [("data", C.c_char_p), ("length", C.c_size_t)]


class GPU_ShaderDesc(C.Structure):
    _fields_ = [("accesses", C.c_void_p), ("accesses_count", C.c_uint32), ("glsl_debug_filepath", GPU_String),
                ("glsl_includer", C.c_void_p), ("glsl_includer_ctx", C.c_void_p), ("spirv", GPU_String), ("glsl", GPU_String)]


class GPU_GLSLError(C.Structure):
    _fields_ = [("shader_stage", C.c_int), ("line", C.c_uint32), ("error_message", GPU_String)]


class GPU_GLSLErrorArray(C.Structure):
    _fields_ = [("data", C.POINTER(GPU_GLSLError)), ("length", C.c_uint32)]


class PBR_IBLMaps(C.Structure):
    _fields_ = [("irradiance_map", C.POINTER(GPU_Texture)), ("brdf_lut", C.POINTER(GPU_Texture)),
                ("tex_specular_env_map", C.POINTER(GPU_Texture))]


class PBR_WorkUnit(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("mip", C.c_uint32), ("face0", C.c_uint32), ("face1", C.c_uint32),
                ("row0", C.c_uint32), ("row1", C.c_uint32), ("cost", C.c_double)]


class PBR_XferRange(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("bytes", C.c_uint64), ("peer", C.c_int)]


class PBR_Globals(C.Structure):
    _fields_ = [(n, C.c_float * 16) for n in ("clip_space_from_world", "clip_space_from_view", "world_space_from_clip",
                                              "view_space_from_clip", "view_space_from_world", "world_space_from_view",
                                              "sun_space_from_world", "old_clip_space_from_world")] + [
        ("sun_direction", C.c_float * 4), ("camera_pos", C.c_float * 3), ("frame_idx_mod_59", C.c_float),
        ("lightgrid_scale", C.c_float), ("visualize_lightgrid", C.c_uint32)]


assert C.sizeof(PBR_Globals) == 552


class PBR_GBuffer(C.Structure):
    _fields_ = [(n, C.POINTER(GPU_Texture)) for n in ("base_color", "normal", "orm", "emissive", "depth", "lighting_result")]


class GPUX_IBLConstants(C.Structure):
    _fields_ = [("mip_level", C.c_int32), ("roughness", C.c_float), ("src_lod", C.c_float), ("sample_count", C.c_int32)]


class PbrkTex2D(C.Structure):
    _fields_ = [("data", C.c_void_p), ("format", C.c_int), ("width", C.c_int), ("height", C.c_int)]


class PbrkTaaArgs(C.Structure):
    _fields_ = [("lighting_result", PbrkTex2D), ("gbuffer_depth", PbrkTex2D), ("gbuffer_velocity", PbrkTex2D),
                ("gbuffer_velocity_prev", PbrkTex2D), ("prev_frame_result", PbrkTex2D), ("out", C.c_void_p),
                ("out_format", C.c_int), ("width", C.c_int), ("height", C.c_int), ("y0", C.c_int), ("y1", C.c_int)]


class PbrkFinalArgs(C.Structure):
    _fields_ = [("src", PbrkTex2D), ("out", C.c_void_p), ("out_format", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("y0", C.c_int), ("y1", C.c_int)]


class PbrkBloomArgs(C.Structure):
    _fields_ = [("src", PbrkTex2D), ("dst", C.c_void_p), ("dst_width", C.c_int), ("dst_height", C.c_int), ("dst_mip_level", C.c_int),
                ("upsample", C.c_int), ("blend_additive", C.c_int), ("y0", C.c_int), ("y1", C.c_int), ("blend_src", C.c_void_p)]


Shade_IBL, Shade_LightShafts, Shade_SunShadows, Shade_VoxelGI = 1, 2, 4, 8
Shade_SH9 = 16                          # GPUX_Shade_SH9Irradiance == PBRK_SHADE_SH9: with Shade_IBL, ambient from 27 SH9 coefficients
PBRK_FMT_RG16F, PBRK_FMT_RG32F, PBRK_FMT_RGBA16F, PBRK_FMT_RGBA32F, PBRK_FMT_R32F, PBRK_FMT_RGBA8UN, PBRK_FMT_BGRA8UN = 1, 2, 3, 4, 5, 6, 7


class PbrkShadeArgs(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("x0", C.c_int), ("x1", C.c_int), ("y0", C.c_int), ("y1", C.c_int),
                ("base_color", C.c_void_p), ("normal", C.c_void_p), ("orm", C.c_void_p), ("emissive", C.c_void_p),
                ("depth", C.c_void_p), ("irradiance_bordered", C.c_void_p), ("irradiance_size", C.c_int),
                ("prefiltered_bordered", C.c_void_p), ("prefiltered_size", C.c_int), ("prefiltered_levels", C.c_int),
                ("lut", C.c_void_p), ("lut_size", C.c_int), ("irradiance_cells", C.c_void_p), ("prefiltered_cells", C.c_void_p),
                ("prefiltered_cells_first", C.c_int), ("lut_cells", C.c_void_p),
                ("sun_depth", C.c_void_p), ("sun_depth_w", C.c_int), ("sun_depth_h", C.c_int),
                ("lightgrid", C.c_void_p), ("lightgrid_size", C.c_int), ("prev_frame", C.c_void_p * 8),
                ("prev_frame_w", C.c_int), ("prev_frame_h", C.c_int), ("prev_frame_levels", C.c_int),
                ("out", C.c_void_p), ("out_format", C.c_int), ("flags", C.c_int),
                ("globals", C.c_float * 138), ("sh9_coef", C.c_void_p)]


class PbrkGridViewArgs(C.Structure):
    _fields_ = [("x0", C.c_int), ("x1", C.c_int), ("y0", C.c_int), ("y1", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("lightgrid", C.c_void_p), ("lightgrid_size", C.c_int), ("out", C.c_void_p), ("out_format", C.c_int),
                ("globals", C.c_float * 138)]


class GPU_TextureView(C.Structure):
    _fields_ = [("texture", C.POINTER(GPU_Texture)), ("mip_level", C.c_uint32)]


class GPU_RenderPassDesc(C.Structure):
    _fields_ = [("color_targets_count", C.c_uint32), ("color_targets", C.POINTER(GPU_TextureView)),
                ("msaa_color_resolve_targets", C.POINTER(GPU_TextureView)), ("width", C.c_uint32), ("height", C.c_uint32),
                ("depth_stencil_target", C.POINTER(GPU_Texture))]


class GPU_GraphicsPipelineDesc(C.Structure):
    _fields_ = [("layout", C.c_void_p), ("render_pass", C.c_void_p), ("vs", GPU_ShaderDesc), ("fs", GPU_ShaderDesc),
                ("vertex_input_formats", C.POINTER(C.c_int)), ("vertex_input_formats_count", C.c_uint32),
                ("enable_depth_test", C.c_bool), ("enable_depth_write", C.c_bool), ("enable_blending", C.c_bool),
                ("blending_mode_additive", C.c_bool), ("enable_conservative_rasterization", C.c_bool), ("cull_mode", C.c_int)]


class PBR_DDSInfoEx(C.Structure):
    _fields_ = [("dxgi_format", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("layers", C.c_uint32), ("level_count", C.c_uint32),
                ("level_offset", (C.c_uint64 * PBR_DDS_MAX_LEVELS) * 6), ("level_size", C.c_uint64 * PBR_DDS_MAX_LEVELS)]


class PBR_DDSInfo(C.Structure):
    _fields_ = [("format", C.c_int), ("width", C.c_uint32), ("height", C.c_uint32), ("level_count", C.c_uint32),
                ("level_offset", C.c_uint64 * PBR_DDS_MAX_LEVELS), ("level_size", C.c_uint64 * PBR_DDS_MAX_LEVELS)]


class PBR_MeshPart(C.Structure):
    _fields_ = [("first_index", C.c_uint32), ("index_count", C.c_uint32)]


CullMode_TwoSided, CullMode_DrawCW, CullMode_DrawCCW = 0, 1, 2
ShaderStage_Vertex, ShaderStage_Fragment, ShaderStage_Compute = 0, 1, 2

TexP = C.POINTER(GPU_Texture)
BufP = C.POINTER(GPU_Buffer)
VP = C.c_void_p
U32 = C.c_uint32

# name -> (restype, argtypes); this table is also what tests use to check the exported symbol set
PROTOTYPES = {
    # --- GPU_* boundary (include/gpu_hip.h) ---
    "GPU_Init": (None, [VP]), "GPU_Deinit": (None, []), "GPU_WaitUntilIdle": (None, []),
    "GPU_SamplerLinearWrap": (VP, []), "GPU_SamplerLinearClamp": (VP, []), "GPU_SamplerLinearMirror": (VP, []),
    "GPU_SamplerNearestClamp": (VP, []), "GPU_SamplerNearestWrap": (VP, []), "GPU_SamplerNearestMirror": (VP, []),
    "GPU_MakeSampler": (VP, [VP]), "GPU_DestroySampler": (None, [VP]),
    "GPU_InitPipelineLayout": (VP, []), "GPU_TextureBinding": (U32, [VP, C.c_char_p]), "GPU_SamplerBinding": (U32, [VP, C.c_char_p]),
    "GPU_BufferBinding": (U32, [VP, C.c_char_p]), "GPU_StorageImageBinding": (U32, [VP, C.c_char_p, C.c_int]),
    "GPU_FinalizePipelineLayout": (None, [VP]), "GPU_DestroyPipelineLayout": (None, [VP]),
    "GPU_MakeDescriptorArena": (VP, []), "GPU_ResetDescriptorArena": (None, [VP]), "GPU_DestroyDescriptorArena": (None, [VP]),
    "GPU_InitDescriptorSet": (VP, [VP, VP]), "GPU_DestroyDescriptorSet": (None, [VP]),
    "GPU_SetTextureBinding": (None, [VP, U32, TexP]), "GPU_SetTextureMipBinding": (None, [VP, U32, TexP, U32]),
    "GPU_SetSamplerBinding": (None, [VP, U32, VP]), "GPU_SetBufferBinding": (None, [VP, U32, BufP]),
    "GPU_SetStorageImageBinding": (None, [VP, U32, TexP, U32]), "GPU_FinalizeDescriptorSet": (None, [VP]),
    "GPU_MakeTexture": (TexP, [C.c_int, U32, U32, U32, C.c_int, VP]), "GPU_DestroyTexture": (None, [TexP]),
    "GPU_MakeBuffer": (BufP, [U32, C.c_int, VP]), "GPU_DestroyBuffer": (None, [BufP]),
    "GPU_SPIRVFromGLSL": (GPU_String, [VP, C.c_int, VP, C.POINTER(GPU_ShaderDesc), C.POINTER(GPU_GLSLErrorArray)]),
    "GPU_JoinGLSLErrorString": (GPU_String, [VP, GPU_GLSLErrorArray]),
    "GPU_MakeRenderPass": (VP, [VP]), "GPU_DestroyRenderPass": (None, [VP]),
    "GPU_MakeGraphicsPipeline": (VP, [VP]), "GPU_DestroyGraphicsPipeline": (None, [VP]),
    "GPU_MakeComputePipeline": (VP, [VP, C.POINTER(GPU_ShaderDesc)]), "GPU_DestroyComputePipeline": (None, [VP]),
    "GPU_MakeGraph": (VP, []), "GPU_GraphSubmit": (None, [VP]), "GPU_GraphWait": (None, [VP]), "GPU_DestroyGraph": (None, [VP]),
    "GPU_MakeSwapchainGraphs": (None, [U32, C.POINTER(VP)]), "GPU_GetBackbuffer": (TexP, [VP]),
    "GPU_OpBindComputePipeline": (None, [VP, VP]), "GPU_OpBindComputeDescriptorSet": (None, [VP, VP]),
    "GPU_OpPushGraphicsConstants": (None, [VP, VP, VP, U32]), "GPU_OpPushComputeConstants": (None, [VP, VP, VP, U32]),
    "GPU_OpDispatch": (None, [VP, U32, U32, U32]),
    "GPU_OpPrepareRenderPass": (None, [VP, VP]), "GPU_OpPrepareDrawParams": (U32, [VP, VP, VP]),
    "GPU_OpBeginRenderPass": (None, [VP]), "GPU_OpEndRenderPass": (None, [VP]), "GPU_OpBindDrawParams": (None, [VP, U32]),
    "GPU_OpDraw": (None, [VP, U32, U32, U32, U32]), "GPU_OpDrawIndexed": (None, [VP, U32, U32, U32, U32, U32]),
    "GPU_OpBindVertexBuffer": (None, [VP, BufP]), "GPU_OpBindIndexBuffer": (None, [VP, BufP]),
    "GPU_OpCopyBufferToBuffer": (None, [VP, BufP, BufP, U32, U32, U32]),
    "GPU_OpCopyBufferToTexture": (None, [VP, BufP, TexP, U32, U32, U32]), "GPU_OpCopyTextureToBuffer": (None, [VP, TexP, BufP]),
    "GPU_OpBlit": (None, [VP, VP]), "GPU_OpGenerateMipmaps": (None, [VP, TexP]),
    "GPU_OpClearColorF": (None, [VP, TexP, U32, C.c_float, C.c_float, C.c_float, C.c_float]),
    "GPU_OpClearColorI": (None, [VP, TexP, U32, U32, U32, U32, U32]), "GPU_OpClearDepthStencil": (None, [VP, TexP, U32]),
    # --- GPUX_* extensions (include/gpux.h) ---
    "GPUX_GetFormatInfo": (None, None),
    "GPUX_SetDevice": (None, [C.c_int]), "GPUX_GetDevice": (C.c_int, []), "GPUX_SetErrorHandler": (None, [VP, VP]),
    "GPUX_BackendName": (C.c_char_p, []), "GPUX_OpDispatchRows": (None, [VP, U32, U32, U32, U32]),
    "GPUX_OpDispatchLines": (None, [VP, U32, U32, U32, U32]),
    "GPUX_SetShadeFlags": (None, [VP, C.c_int]), "GPUX_GetShadeFlags": (C.c_int, [VP]), "GPUX_SetShadeSH9": (None, [VP, BufP, U32]),
    "GPUX_OpDrawRows": (None, [VP, U32, U32]),
    "GPUX_OpCopyTextureMipToBuffer": (None, [VP, TexP, U32, BufP, U32]), "GPUX_OpCopyBufferToTextureMip": (None, [VP, BufP, U32, TexP, U32]),
    "GPUX_OpCopyDecodedTextureMipToBuffer": (None, [VP, TexP, U32, BufP, U32]),
    "GPUX_FoldedBlitCount": (C.c_uint64, []), "GPUX_SetGraphOverlap": (None, [C.c_int]), "GPUX_OverlappedSubmitCount": (C.c_uint64, []), "GPUX_TextureMipBytes": (C.c_uint64, [TexP, U32]), "GPUX_TextureDevicePtr": (VP, [TexP, U32]), "GPUX_BufferDevicePtr": (VP, [BufP]),
    "GPUX_MakeTextureExternal": (TexP, [C.c_int, U32, U32, U32, C.c_int, VP, C.c_uint64]),
    "GPUX_InvalidateTexture": (None, [TexP]),
    "GPUX_TextureTotalBytes": (C.c_uint64, [TexP]), "GPUX_TextureMipOffset": (C.c_uint64, [TexP, U32]),
    "GPUX_MakeCubemapFromEquirect": (TexP, [VP, U32, U32, U32, C.c_int]),
    "GPUX_RasterRejectedTriangles": (C.c_uint64, []), "GPUX_VoxelizeFragments": (C.c_uint64, []),
    "GPUX_GraphStream": (VP, [VP]), "GPUX_EnableOpTiming": (None, [C.c_int]), "GPUX_SetTileStreams": (None, [C.c_int]), "GPUX_SetLevelOverlap": (None, [C.c_int]), "GPUX_SetLevelStreams": (None, [C.c_int]), "GPUX_LevelOverlapCount": (U32, []), "GPUX_GraphTimedOpCount": (U32, [VP]),
    "GPUX_GraphTimedOpName": (C.c_char_p, [VP, U32]), "GPUX_GraphTimedOpMs": (C.c_float, [VP, U32]), "GPUX_GraphSpanMs": (C.c_float, [VP]),
    # --- host layer (include/pbr_host.h) ---
    "PBR_DecodeHDR": (VP, [VP, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]),
    "PBR_MakeTextureFromHDRIMemory": (TexP, [VP, C.c_size_t]), "PBR_MakeTextureFromHDRIFile": (TexP, [C.c_char_p]),
    "PBR_MakeTextureFromEquirectHDRIMemory": (TexP, [VP, C.c_size_t, U32]), "PBR_MakeTextureFromEquirectHDRIFile": (TexP, [C.c_char_p, U32]),
    "PBR_EncodeHDR": (VP, [VP, C.c_int, C.c_int, C.POINTER(C.c_size_t)]), "PBR_WriteHDRFile": (C.c_int, [C.c_char_p, VP, C.c_int, C.c_int]),
    "PBR_WriteCubeStripHDR": (C.c_int, [C.c_char_p, TexP, U32]),
    "PBR_MakeIBLMaps": (None, [C.POINTER(PBR_IBLMaps), U32, U32, U32]), "PBR_DestroyIBLMaps": (None, [C.POINTER(PBR_IBLMaps)]),
    "PBR_GenIrradianceMap": (None, [TexP, TexP]), "PBR_GenPrefilteredEnvMap": (None, [TexP, TexP, U32]),
    "PBR_GenBRDFIntegrationMap": (None, [TexP]),
    "PBR_MakeIBLPipelines": (VP, []), "PBR_DestroyIBLPipelines": (None, [VP]),
    "PBR_RecordUnits": (None, [VP, VP, VP, TexP, C.POINTER(PBR_IBLMaps), C.POINTER(PBR_WorkUnit), U32]),
    "PBR_PartitionIBL": (U32, [U32, U32, U32, U32, C.c_int, C.c_int, C.POINTER(PBR_WorkUnit), U32]),
    "PBR_ExchangeRanges": (C.c_int, [VP, VP, VP, U32, VP, U32]),
    "PBR_SetRcclLibrary": (C.c_int, [C.c_char_p]), "PBR_RcclInfo": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_char_p)]),
    "PBR_CommInfo": (C.c_int, [VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "PBR_UnitByteRange": (C.c_int, [C.POINTER(PBR_IBLMaps), C.POINTER(PBR_WorkUnit), C.POINTER(TexP), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "PBR_GatherUnits": (C.c_int64, [VP, VP, C.c_int, C.c_int, C.c_int, C.POINTER(PBR_IBLMaps), U32, U32]),
    "GPUX_SetGraphReplay": (None, [C.c_int]),
    "GPUX_GraphReplayStats": (None, [VP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "PBR_GatherUnitsMasked": (C.c_int64, [VP, VP, C.c_int, C.c_int, C.c_int, C.POINTER(PBR_IBLMaps), U32, U32, U32]),
    "PBR_GatherPlan": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.POINTER(PBR_IBLMaps), U32, U32, U32, VP, U32]),
    "PBR_SelectUnits": (U32, [C.POINTER(PBR_WorkUnit), U32, U32, C.POINTER(PBR_WorkUnit)]),
    "PBR_RunPartitionedIBL": (C.c_int64, [VP, VP, VP, VP, TexP, C.POINTER(PBR_IBLMaps), VP, C.c_int, C.c_int, C.c_int, U32, U32]),
    "PBR_BandRows": (None, [U32, C.c_int, C.c_int, C.POINTER(U32), C.POINTER(U32)]),
    "PBR_GatherBands": (C.c_int64, [VP, VP, C.c_int, C.c_int, C.c_int, TexP]),
    "PBR_FillGlobals": (None, [C.POINTER(PBR_Globals), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float,
                               C.c_float, C.c_float, C.c_float, C.c_float, U32]),
    "PBR_MakeGBuffer": (None, [C.POINTER(PBR_GBuffer), U32, U32, C.c_int]), "PBR_DestroyGBuffer": (None, [C.POINTER(PBR_GBuffer)]),
    "PBR_MakeLightingPass": (VP, [C.POINTER(PBR_GBuffer), C.POINTER(PBR_IBLMaps), U32, U32]), "PBR_DestroyLightingPass": (None, [VP]),
    "PBR_MakeLightingPassEx": (VP, [C.POINTER(PBR_GBuffer), C.POINTER(PBR_IBLMaps), U32, U32, TexP]),
    "PBR_MakeLightingPassLive": (VP, [C.POINTER(PBR_GBuffer), C.POINTER(PBR_IBLMaps), U32, U32, TexP, TexP, TexP]),
    "PBR_LightingGlobalsBuffer": (BufP, [VP]), "PBR_LightingPipeline": (VP, [VP]),
    "PBR_RecordLightingPass": (None, [VP, VP, C.POINTER(PBR_Globals), U32, U32]), "PBR_LightingUseSH9": (None, [VP, BufP, U32]),
    "PBR_MakePostProcess": (VP, [C.POINTER(PBR_GBuffer), U32, U32, C.c_int]), "PBR_DestroyPostProcess": (None, [VP]),
    "PBR_PostVelocity": (TexP, [VP, U32]), "PBR_PostTaaOutput": (TexP, [VP, U32]), "PBR_PostBackbuffer": (TexP, [VP]),
    "PBR_RecordBloom": (None, [VP, VP, U32]), "PBR_RecordFinalPostProcessBloom": (None, [VP, VP, U32]),
    "PBR_PostBloomDownscale": (TexP, [VP]), "PBR_PostBloomUpscale": (TexP, [VP]), "PBR_PostBloomPassCount": (U32, [VP]),
    "PBR_RecordTaaResolve": (None, [VP, VP, U32]), "PBR_RecordTaaResolveRows": (None, [VP, VP, U32, U32, U32]), "PBR_RecordFinalPostProcess": (None, [VP, VP, U32]),
    "PBR_MakeMesh": (VP, [VP, U32, VP, U32, C.POINTER(PBR_MeshPart), U32]), "PBR_DestroyMesh": (None, [VP]),
    "PBR_MeshVertexBuffer": (BufP, [VP]), "PBR_MeshIndexBuffer": (BufP, [VP]), "PBR_MeshPartCount": (U32, [VP]),
    "PBR_MakeSunDepthPass": (VP, [U32]), "PBR_DestroySunDepthPass": (None, [VP]), "PBR_SunDepthTexture": (TexP, [VP]),
    "PBR_SunDepthGlobalsBuffer": (BufP, [VP]), "PBR_SunDepthPipeline": (VP, [VP]), "PBR_SunDepthRenderPass": (VP, [VP]),
    "PBR_SunDepthLayout": (VP, [VP]), "PBR_SunDepthDescriptorSet": (VP, [VP]),
    "PBR_RecordSunDepthPass": (None, [VP, VP, VP, C.POINTER(PBR_Globals)]),
    "PBR_MakeMaterial": (VP, [U32, VP, VP, VP, VP]), "PBR_DestroyMaterial": (None, [VP]), "PBR_MaterialTexture": (TexP, [VP, U32]),
    "PBR_MeshSetPartMaterial": (None, [VP, U32, VP]),
    "PBR_MakeMaterialFromTextures": (VP, [C.POINTER(TexP)]),
    "PBR_ParseDDS": (C.c_int, [VP, C.c_size_t, C.POINTER(PBR_DDSInfo)]), "PBR_DDSErrorString": (C.c_char_p, [C.c_int]),
    "PBR_MakeTextureFromDDSMemory": (TexP, [VP, C.c_size_t, U32]), "PBR_MakeTextureFromDDSFile": (TexP, [C.c_char_p, U32]),
    "PBR_MakeGeometryPass": (VP, [C.POINTER(PBR_GBuffer), VP, U32, U32]), "PBR_DestroyGeometryPass": (None, [VP]),
    "PBR_GeometryGlobalsBuffer": (BufP, [VP]), "PBR_GeometryPipeline": (VP, [VP, U32]), "PBR_GeometryRenderPass": (VP, [VP, U32]),
    "PBR_GeometryLayout": (VP, [VP]), "PBR_GeometryDescriptorSet": (VP, [VP, VP]),
    "PBR_RecordGeometryPass": (None, [VP, VP, VP, VP, C.POINTER(PBR_Globals), C.POINTER(C.c_float), C.POINTER(C.c_float), U32]),
    "PBR_MakeVoxelizePass": (VP, [VP, VP]), "PBR_DestroyVoxelizePass": (None, [VP]), "PBR_VoxelizeGlobalsBuffer": (BufP, [VP]),
    "PBR_VoxelizePipeline": (VP, [VP]), "PBR_VoxelizeRenderPass": (VP, [VP]), "PBR_VoxelizeLayout": (VP, [VP]),
    "PBR_VoxelizeShadowSampler": (VP, [VP]), "PBR_VoxelizeDescriptorSet": (VP, [VP, VP, VP]),
    "PBR_RecordVoxelizePass": (None, [VP, VP, VP, C.POINTER(PBR_Globals)]),
    "PBR_MakeLightgrid": (VP, [U32]), "PBR_DestroyLightgrid": (None, [VP]), "PBR_LightgridTexture": (TexP, [VP]),
    "PBR_LightgridSweepDirection": (U32, [VP]), "PBR_RecordLightgridClear": (None, [VP, VP]),
    "PBR_RecordLightgridSweep": (None, [VP, VP]), "PBR_RecordLightgridSweepLines": (None, [VP, VP, U32, U32, U32, U32, U32]),
    # --- low-level kernel ABI (include/pbr_kernels.h) ---
    "pbrk_level_offset": (C.c_size_t, [C.c_int, C.c_int]), "pbrk_pyramid_texels": (C.c_size_t, [C.c_int, C.c_int]),
    "pbrk_bordered_level_offset": (C.c_size_t, [C.c_int, C.c_int]), "pbrk_bordered_pyramid_texels": (C.c_size_t, [C.c_int, C.c_int]),
    "pbrk_mip_count": (C.c_int, [C.c_int, C.c_int]),
    "pbrk_host_sample_angles": (None, [C.c_int, VP]), "pbrk_host_prefilter_table": (C.c_int, [C.c_int, C.c_float, VP, C.POINTER(C.c_float)]),
    "pbrk_host_irradiance_table": (C.c_int, [C.c_int, VP]),
    "pbrk_mip_chain": (C.c_int, [VP, C.c_int, C.c_int, VP]),
    "pbrk_level_minmax": (C.c_int, [VP, C.c_size_t, VP, VP]),
    "GPUX_SetPrefilterTolerance": (None, [C.c_float]), "GPUX_PrefilterKeptSamples": (C.c_int, [U32]),
    "pbrk_set_cube_sampler_snap": (None, [C.c_int]), "pbrk_get_cube_sampler_snap": (C.c_int, []), "pbrk_box_downsample": (C.c_int, [VP, C.c_int, VP, C.c_int, VP]),
    "pbrk_blit_linear": (C.c_int, [VP, C.c_int, C.c_int, VP, C.c_int, C.c_int, C.c_int, VP]),
    "pbrk_fill_pattern": (C.c_int, [VP, C.c_ulonglong, VP, C.c_int, VP]),
    "pbrk_bloom_set_thresholds": (None, [C.c_longlong, C.c_longlong]),
    "pbrk_mc_set_kernels": (None, [C.c_int, C.c_int]), "pbrk_shade_set_fast": (None, [C.c_int]), "pbrk_shade_last_kernel": (C.c_int, []),
    "pbrk_border_build": (C.c_int, [VP, VP, C.c_int, C.c_int, VP]),
    "pbrk_border_build_range": (C.c_int, [VP, VP, C.c_int, C.c_int, C.c_int, C.c_int, VP]),
    "pbrk_debug_sample": (C.c_int, [C.c_int, VP, C.c_int, C.c_int, C.c_int, VP, C.c_int, VP, VP]),
    "pbrk_bloom_pass": (C.c_int, [VP, VP]),
    "pbrk_taa_resolve": (C.c_int, [VP, VP]), "pbrk_final_post_process": (C.c_int, [VP, VP]),
    "pbrk_lightgrid_sweep": (C.c_int, [VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP]),
    "pbrk_brdf_lut": (C.c_int, [VP, C.c_int, C.c_int, C.c_int, VP, VP, C.c_int, C.c_int, VP]),
    "pbrk_prefilter_copy": (C.c_int, [VP, C.c_int, VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP]),
    "pbrk_mc_filter": (C.c_int, [VP, VP, C.c_int, VP, C.c_int, C.c_float, C.c_float, VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP]),
    "pbrk_cells_bytes": (C.c_size_t, [C.c_int]), "pbrk_cells_build": (C.c_int, [VP, C.c_int, VP, VP]),
    "pbrk_shade": (C.c_int, [C.POINTER(PbrkShadeArgs), VP]),
    "pbrk_lightgrid_view": (C.c_int, [C.POINTER(PbrkGridViewArgs), VP]),
    "pbrk_mc_region_stats": (C.c_int, [C.POINTER(C.c_uint64), C.c_int]),
    "pbrk_mc_region_flag_stats": (C.c_int, [C.POINTER(C.c_uint64)]), "pbrk_mc_region_window_stats": (C.c_int, [C.POINTER(C.c_uint64)]),
    "pbrk_mc_region_skip_stats": (C.c_int, [C.POINTER(C.c_uint64)]), "pbrk_mc_set_absorb": (None, [C.c_int]),
    "pbrk_mc_set_runs": (None, [C.c_int]), "pbrk_mc_region_order": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "pbrk_mc_set_prologue": (None, [C.c_int]), "pbrk_mc_set_launch_cut": (None, [C.c_int]),
    "pbrk_mc_launch_cut": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.c_uint, C.c_uint, C.POINTER(C.c_int)]),
    "pbrk_mc_launch_cut_stats": (C.c_int, [C.POINTER(C.c_int)]),
    "pbrk_mc_launch_cut_slices": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_uint, C.c_uint, C.POINTER(C.c_int)]),
    "pbrk_mc_set_tile32": (None, [C.c_int]),
    "pbrk_mc_set_fold": (None, [C.c_int]), "pbrk_mc_last_fold": (C.c_int, []),
    "pbrk_mc_set_net": (None, [C.c_int]), "pbrk_mc_last_net": (C.c_int, []),
    "pbrk_mc_mono_slices": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "pbrk_mc_set_resident": (None, [C.c_int]), "pbrk_mc_resident_stats": (C.c_int, [C.POINTER(C.c_uint64)]),
    "pbrk_mc_region_phase_stats": (C.c_int, [C.POINTER(C.c_uint64)]),
    "pbrk_mc_table_register": (C.c_int, [VP, C.c_int]), "pbrk_mc_table_unregister": (C.c_int, [VP]),
    "pbrk_mc_set_bin_cache": (None, [C.c_int]), "pbrk_mc_set_bin_cache_budget": (None, [C.c_size_t]), "pbrk_mc_bin_cache_clear": (None, []),
    "pbrk_mc_bin_cache_stats": (None, [C.POINTER(C.c_uint64)]),
    "pbrk_mc_set_exact_bins": (None, [C.c_int]), "pbrk_mc_last_exact_bins": (C.c_int, []),
    "pbrk_mc_exact_bins_stats": (C.c_int, [C.POINTER(C.c_uint64), C.c_int]),
    "pbrk_mc_plan": (C.c_int, [C.c_int] * 9 + [VP]),
    "pbrk_mc_tile_of_block": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "pbrk_mc_bin_window_eligible": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "pbrk_lut_cells_build": (C.c_int, [VP, C.c_int, VP, VP]),
    "pbrk_equirect_to_cube": (C.c_int, [VP, C.c_int, C.c_int, VP, C.c_int, VP]),
    "pbrk_raster_scratch_bytes": (C.c_size_t, [U32, C.c_int, C.c_int]),
    "pbrk_raster_setup": (C.c_int, [VP, VP]), "pbrk_raster_tiles": (C.c_int, [VP, VP]),
    "pbrk_geometry_scratch_bytes": (C.c_size_t, [U32, C.c_int, C.c_int]),
    "pbrk_geometry_setup": (C.c_int, [VP, VP]), "pbrk_geometry_tiles": (C.c_int, [VP, VP]),
    "pbrk_voxelize_scratch_bytes": (C.c_size_t, [U32, C.c_int, C.c_int]),
    "pbrk_voxelize_cover": (C.c_int, [VP, VP]), "pbrk_voxelize_resolve": (C.c_int, [VP, VP]),
    "pbrk_mip_chain_rgba8": (C.c_int, [VP, C.c_int, C.c_int, C.c_int, VP]),
    "pbrk_bc_decode": (C.c_int, [C.c_int, VP, C.c_int, C.c_int, VP, VP]),
    # --- K17: SH9 projection / irradiance ---
    "pbrk_sh9_scratch_bytes": (C.c_size_t, [C.c_int]),
    "pbrk_sh9_project": (C.c_int, [VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP, VP, VP]),
    "pbrk_sh9_irradiance": (C.c_int, [VP, VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP]),
    "GPUX_OpProjectSH9": (None, [VP, TexP, U32, U32, U32, U32, U32, BufP, U32]),
    "GPUX_OpIrradianceFromSH9": (None, [VP, BufP, U32, TexP, U32]),
    "PBR_ProjectSH9": (C.c_int, [TexP, U32, C.POINTER(C.c_double)]), "PBR_GenIrradianceMapSH": (None, [TexP, U32, TexP]),
    "PBR_EvalSH9Irradiance": (None, [C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "PBR_WriteSH9File": (C.c_int, [C.c_char_p, C.POINTER(C.c_double)]), "PBR_ReadSH9File": (C.c_int, [C.c_char_p, C.POINTER(C.c_double)]),
    # --- K18: BC6H encode, .dds output ---
    "pbrk_bc6h_level_bytes": (C.c_uint64, [C.c_int, C.c_int, C.c_int]),
    "pbrk_bc6h_encode": (C.c_int, [VP, C.c_int, C.c_int, C.c_int, C.c_int, VP, VP]),
    "GPUX_OpEncodeBC6H": (None, [VP, TexP, U32, BufP, U32]), "GPUX_BC6HMipBytes": (C.c_uint64, [TexP, U32]),
    "pbrk_bc6h_encode2": (C.c_int, [VP, C.c_int, C.c_int, C.c_int, C.c_int, VP, VP]),
    "GPUX_OpEncodeBC6HEx": (None, [VP, TexP, U32, BufP, U32, U32]),
    "PBR_ParseDDSEx": (C.c_int, [VP, C.c_size_t, C.POINTER(PBR_DDSInfoEx)]),
    "PBR_BuildDDSHeader": (C.c_uint64, [U32, U32, U32, U32, U32, C.POINTER(C.c_uint8), C.POINTER(PBR_DDSInfoEx)]),
    "PBR_EncodeTextureDDS": (VP, [TexP, U32, U32, C.c_int, C.POINTER(C.c_size_t)]),
    "PBR_WriteTextureDDS": (C.c_int, [C.c_char_p, TexP, U32, U32, C.c_int]),
    "PBR_MakeTextureFromFloatDDSMemory": (TexP, [VP, C.c_size_t]), "PBR_MakeTextureFromFloatDDSFile": (TexP, [C.c_char_p]),
    # --- K19: BC6H decode, loading BC6H .dds files ---
    "pbrk_bc6h_decode": (C.c_int, [VP, C.c_int, C.c_int, C.c_int, VP, C.c_int, VP]),
    "GPUX_OpDecodeBC6H": (None, [VP, BufP, U32, TexP, U32]),
    "PBR_MakeTextureFromBC6HDDSMemory": (TexP, [VP, C.c_size_t, C.c_int]), "PBR_MakeTextureFromBC6HDDSFile": (TexP, [C.c_char_p, C.c_int]),
    "PBR_DecodeBC6HBlocks": (None, [VP, U32, U32, C.POINTER(C.c_uint16)]),
    # --- K20: cube level -> lat-long panorama ---
    "pbrk_cube_to_panorama": (C.c_int, [VP, C.c_int, VP, VP, C.c_int, C.c_int, C.c_int, VP]),
    "GPUX_OpCubeToPanorama": (None, [VP, TexP, U32, TexP, U32]),
    "GPUX_PanoramaDirections": (C.c_int, [U32, U32, C.POINTER(C.c_float)]),
    "PBR_MakePanoramaFromCube": (TexP, [TexP, U32, U32, U32, C.c_int]),
    "PBR_WritePanoramaHDR": (C.c_int, [C.c_char_p, TexP, U32, U32, U32]),
    # --- K21: GGX importance-sampled prefilter ---
    "pbrk_prefilter_ggx": (C.c_int, [VP, VP, C.c_int, C.c_float, VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP]),
    "GPUX_OpPrefilterGGX": (None, [VP, TexP, TexP, U32, C.c_float, U32, C.c_float, U32, U32, U32, U32]),
    "GPUX_PrefilterGGXSamples": (C.c_int, [C.c_float, U32, U32, U32, C.c_float, C.POINTER(C.c_float), C.POINTER(U32), C.POINTER(C.c_float)]),
    "PBR_GenPrefilteredEnvMapGGX": (None, [TexP, TexP, U32, U32]),
    "PBR_RecordPrefilterLevel": (None, [VP, VP, VP, TexP, TexP, U32]),
    # --- K22: GGX split-sum BRDF LUT ---
    "pbrk_brdf_lut_ggx": (C.c_int, [VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP, C.c_int, C.c_int, VP]),
    "GPUX_OpBrdfLutGGX": (None, [VP, TexP, U32, U32, U32, U32]),
    "GPUX_BrdfLutGGXSamples": (C.c_int, [U32, C.POINTER(C.c_float)]),
    "PBR_GenBRDFIntegrationMapGGX": (None, [TexP, U32, U32]),
}

_LIB = None


def lib():
    """Load libgpu_hip.so.  No fallback: a missing library is a hard error."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C {os.path.join(PKG_ROOT, 'csrc')}` "
                           "(or __graft_entry__.build()); there is no CPU fallback for the HIP path")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(L, name)
        if args is not None:
            fn.restype = res
            fn.argtypes = args
    _LIB = L
    return L


# ---- conveniences used by tests / bench ------------------------------------------------------
_FMT_NP = {Format_RGBA32F: (np.float32, 4), Format_RG32F: (np.float32, 2), Format_RG16F: (np.float16, 2),
           Format_RGBA16F: (np.float16, 4), Format_RGBA8UN: (np.uint8, 4), Format_BGRA8UN: (np.uint8, 4), Format_D32F_Or_X8D24UN: (np.float32, 1),
           Format_R32F: (np.float32, 1)}


def init(device=None):
    L = lib()
    if device is not None:
        L.GPUX_SetDevice(int(device))
    L.GPU_Init(None)
    return L


def make_texture(fmt, w, h, flags, data=None, depth=1):
    L = lib()
    ptr = None
    if data is not None:
        data = np.ascontiguousarray(data)
        ptr = data.ctypes.data_as(VP)
    t = L.GPU_MakeTexture(fmt, w, h, depth, flags, ptr)
    if not t:
        raise RuntimeError("GPU_MakeTexture failed")
    return t


def upload_mip(tex, mip, array):
    """Host array -> all layers of one mip (staging buffer + GPUX_OpCopyBufferToTextureMip)."""
    L = lib()
    array = np.ascontiguousarray(array)
    nbytes = L.GPUX_TextureMipBytes(tex, mip)
    assert array.nbytes == nbytes, (array.nbytes, nbytes)
    buf = L.GPU_MakeBuffer(nbytes, BufferFlag_CPU, array.ctypes.data_as(VP))
    g = L.GPU_MakeGraph()
    L.GPUX_OpCopyBufferToTextureMip(g, buf, 0, tex, mip)
    L.GPU_GraphSubmit(g)
    L.GPU_GraphWait(g)
    L.GPU_DestroyGraph(g)
    L.GPU_DestroyBuffer(buf)


def read_mip(tex, mip=0):
    """All layers of one mip -> numpy array [layers][h][w][c] (squeezed for single-layer textures; [d][h][w][c] for 3-D)."""
    L = lib()
    t = tex.contents
    nbytes = L.GPUX_TextureMipBytes(tex, mip)
    buf = L.GPU_MakeBuffer(nbytes, BufferFlag_CPU, None)
    g = L.GPU_MakeGraph()
    L.GPUX_OpCopyTextureMipToBuffer(g, tex, mip, buf, 0)
    L.GPU_GraphSubmit(g)
    L.GPU_GraphWait(g)
    dt, ch = _FMT_NP[t.format]
    w, h = max(1, t.width >> mip), max(1, t.height >> mip)
    raw = (C.c_char * nbytes).from_address(buf.contents.data)
    d = max(1, t.depth >> mip)
    arr = np.frombuffer(raw, dtype=dt).reshape(t.layer_count * d, h, w, ch).copy()
    L.GPU_DestroyGraph(g)
    L.GPU_DestroyBuffer(buf)
    return arr if (t.layer_count > 1 or d > 1) else arr[0]


def _read_back(record, nbytes):
    L = lib()
    buf = L.GPU_MakeBuffer(nbytes, BufferFlag_CPU, None)
    g = L.GPU_MakeGraph()
    record(g, buf)
    L.GPU_GraphSubmit(g)
    L.GPU_GraphWait(g)
    raw = C.string_at(buf.contents.data, nbytes)
    L.GPU_DestroyGraph(g)
    L.GPU_DestroyBuffer(buf)
    return raw


def read_mip_bytes(tex, mip=0):
    """One mip as the texture stores it (for a BC texture: its blocks) -> bytes."""
    L = lib()
    return _read_back(lambda g, buf: L.GPUX_OpCopyTextureMipToBuffer(g, tex, mip, buf, 0), L.GPUX_TextureMipBytes(tex, mip))


def read_decoded_mip(tex, mip=0):
    """One level of a BC texture's decoded image (K15) -> uint8 [h][w][4]."""
    L = lib()
    t = tex.contents
    w, h = max(1, t.width >> mip), max(1, t.height >> mip)
    raw = _read_back(lambda g, buf: L.GPUX_OpCopyDecodedTextureMipToBuffer(g, tex, mip, buf, 0), w * h * 4)
    return np.frombuffer(raw, np.uint8).reshape(h, w, 4).copy()


def project_sh9(tex, mip, faces=(0, 6), rows=None):
    """SH9 coefficients (K17) of rows [rows) of faces [faces) of one level of an RGBA32F cube -> float64 [9][3] (k, channel).
    A sub-range gives that range's partial sum; rows=None is the whole level."""
    L = lib()
    n = max(1, tex.contents.width >> mip)
    r0, r1 = (0, n) if rows is None else rows
    raw = _read_back(lambda g, buf: L.GPUX_OpProjectSH9(g, tex, mip, faces[0], faces[1], r0, r1, buf, 0), 216)
    return np.frombuffer(raw, np.float64).reshape(9, 3).copy()


def irradiance_from_sh9(coef, tex, mip=0):
    """Writes one level of an RGBA32F cube with the irradiance (E / 2 pi, alpha 0, not clamped) of 27 SH9 coefficients."""
    L = lib()
    coef = np.ascontiguousarray(coef, np.float64).reshape(27)
    buf = L.GPU_MakeBuffer(216, BufferFlag_CPU, coef.ctypes.data_as(VP))
    g = L.GPU_MakeGraph()
    L.GPUX_OpIrradianceFromSH9(g, buf, 0, tex, mip)
    L.GPU_GraphSubmit(g)
    L.GPU_GraphWait(g)
    L.GPU_DestroyGraph(g)
    L.GPU_DestroyBuffer(buf)


def parse_dds(data: bytes):
    """PBR_ParseDDS -> PBR_DDSInfo, or raises ValueError with the parser's reason."""
    info = PBR_DDSInfo()
    rc = lib().PBR_ParseDDS(data, len(data), C.byref(info))
    if rc != 0:
        raise ValueError(lib().PBR_DDSErrorString(rc).decode())
    return info


def make_texture_from_dds_file(path, flags=0):
    t = lib().PBR_MakeTextureFromDDSFile(os.fsencode(path), flags)
    if not t:
        raise RuntimeError("PBR_MakeTextureFromDDSFile failed")
    return t


def make_material_from_textures(textures):
    """four GPU_Texture* (or None: the 1 x 1 dummy of that slot) -> PBR_Material* that does not own them."""
    arr = (TexP * 4)(*[t if t is not None else TexP() for t in textures])
    m = lib().PBR_MakeMaterialFromTextures(arr)
    if not m:
        raise RuntimeError("PBR_MakeMaterialFromTextures failed")
    return m


def fill_globals(pos, ori=None, fov=75.0, aspect=16.0 / 9.0, near=0.02, far=1.0e4, sun_angle=(56.5, 97.0), frame_idx=0):
    g = PBR_Globals()
    p = (C.c_float * 3)(*[float(v) for v in pos])
    o = None if ori is None else (C.c_float * 4)(*[float(v) for v in ori])
    lib().PBR_FillGlobals(C.byref(g), p, o, fov, aspect, near, far, sun_angle[0], sun_angle[1], frame_idx)
    return g


def make_mesh(vertices, indices, parts):
    """vertices float32 [n][11] (or [n][3]: padded to the reference's 44-B Vertex), indices uint32, parts [(first_index, index_count)]
    -> PBR_Mesh* (GPU vertex + index buffers, asset_import.cpp:172-173)."""
    v = np.asarray(vertices, np.float32)
    if v.ndim == 2 and v.shape[1] == 3:
        v = np.concatenate([v, np.zeros((len(v), 8), np.float32)], 1)
    v = np.ascontiguousarray(v)
    assert v.ndim == 2 and v.shape[1] == 11, v.shape
    ix = np.ascontiguousarray(indices, np.uint32)
    pa = (PBR_MeshPart * max(1, len(parts)))(*[PBR_MeshPart(int(a), int(b)) for a, b in parts])
    m = lib().PBR_MakeMesh(v.ctypes.data_as(VP), len(v), ix.ctypes.data_as(VP), len(ix), pa, len(parts))
    if not m:
        raise RuntimeError("PBR_MakeMesh failed")
    return m


def make_material(images):
    """images: four uint8 [size][size][4] level-0 images (base colour, normal, ORM, emissive) -> PBR_Material* with generated mips."""
    imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
    size = imgs[0].shape[0]
    assert len(imgs) == 4 and all(im.shape == (size, size, 4) for im in imgs)
    m = lib().PBR_MakeMaterial(size, *[im.ctypes.data_as(VP) for im in imgs])
    if not m:
        raise RuntimeError("PBR_MakeMaterial failed")
    return m


def make_voxelize_pass(lightgrid, sun_depth_pass):
    """PBR_Lightgrid*, PBR_SunDepthPass* -> PBR_VoxelizePass* (K14: lightgrid_voxelize.glsl drawn into the grid, shadowed by the sun map)."""
    p = lib().PBR_MakeVoxelizePass(lightgrid, sun_depth_pass)
    if not p:
        raise RuntimeError("PBR_MakeVoxelizePass failed")
    return p


def partition(specular_size, min_size, irradiance_size, env_size, world, rank):
    L = lib()
    n = L.PBR_PartitionIBL(specular_size, min_size, irradiance_size, env_size, world, rank, None, 0)
    arr = (PBR_WorkUnit * max(1, n))()
    m = L.PBR_PartitionIBL(specular_size, min_size, irradiance_size, env_size, world, rank, arr, n)
    assert m == n
    return arr, n


# ---- RCCL bootstrap for tests / bench.py (the library itself never creates a communicator: include/pbr_host.h) ----
class NcclUniqueId(C.Structure):
    _fields_ = [("internal", C.c_char * 128)]


_RCCL = None


def rccl_info():
    """(ncclGetVersion code, path of the librccl the C host layer bound) -- PBR_RcclInfo; raises if none can be loaded."""
    ver, path = C.c_int(0), C.c_char_p()
    if lib().PBR_RcclInfo(C.byref(ver), C.byref(path)) != 0:
        raise RuntimeError("no librccl.so.1 could be bound (PBR_RCCL_LIB / PBR_SetRcclLibrary select one explicitly)")
    return int(ver.value), (path.value or b"").decode()


def rccl():
    """The SAME librccl the C host layer calls (PBR_RcclInfo names the file; one copy per process by SONAME), so that a
    communicator made here is valid for PBR_GatherUnits / PBR_GatherBands / PBR_ExchangeRanges."""
    global _RCCL
    if _RCCL is None:
        _, path = rccl_info()
        R = C.CDLL(path or "librccl.so.1")
        R.ncclGetUniqueId.argtypes = [C.POINTER(NcclUniqueId)]; R.ncclGetUniqueId.restype = C.c_int
        R.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, NcclUniqueId, C.c_int]; R.ncclCommInitRank.restype = C.c_int
        R.ncclCommDestroy.argtypes = [C.c_void_p]; R.ncclCommDestroy.restype = C.c_int
        R.ncclGetErrorString.argtypes = [C.c_int]; R.ncclGetErrorString.restype = C.c_char_p
        _RCCL = R
    return _RCCL


def comm_info(comm):
    """(rank count, this rank) as the communicator itself reports them (ncclCommCount / ncclCommUserRank)."""
    n, r = C.c_int(-1), C.c_int(-1)
    if lib().PBR_CommInfo(comm, C.byref(n), C.byref(r)) != 0:
        raise RuntimeError("PBR_CommInfo failed")
    return int(n.value), int(r.value)


def rccl_unique_id():
    uid = NcclUniqueId()
    rc = rccl().ncclGetUniqueId(C.byref(uid))
    if rc != 0:
        raise RuntimeError("ncclGetUniqueId: " + rccl().ncclGetErrorString(rc).decode())
    return C.string_at(C.byref(uid), 128)              # (a c_char array read as bytes stops at the first NUL)


def rccl_comm_init(world, rank, unique_id: bytes):
    """ncclCommInitRank -> opaque communicator handle (c_void_p) for PBR_GatherUnits / PBR_GatherBands / PBR_ExchangeRanges."""
    uid = NcclUniqueId()
    C.memmove(C.byref(uid), unique_id, 128)
    comm = C.c_void_p()
    rc = rccl().ncclCommInitRank(C.byref(comm), int(world), uid, int(rank))
    if rc != 0:
        raise RuntimeError("ncclCommInitRank: " + rccl().ncclGetErrorString(rc).decode())
    return comm


def rccl_comm_destroy(comm):
    rccl().ncclCommDestroy(comm)


def parse_dds_ex(data: bytes):
    """PBR_ParseDDSEx -> PBR_DDSInfoEx (cubes, float and BC6H formats too), or raises ValueError with the parser's reason."""
    info = PBR_DDSInfoEx()
    rc = lib().PBR_ParseDDSEx(data, len(data), C.byref(info))
    if rc != 0:
        raise ValueError(lib().PBR_DDSErrorString(rc).decode())
    return info


def encode_bc6h(tex, mip=0, quality=GPUX_BC6H_OneRegion):
    """One level (every layer) of an RGBA32F / RGBA16F texture as BC6H_UF16 blocks (K18) -> uint8 [layers * bh * bw][16].
    quality: GPUX_BC6H_OneRegion (mode 11 only) or GPUX_BC6H_TwoRegions (GPUX_OpEncodeBC6HEx)."""
    L = lib()
    nbytes = L.GPUX_BC6HMipBytes(tex, mip)
    if nbytes == 0:
        raise ValueError("encode_bc6h: not a level of a 2-D or cube RGBA32F / RGBA16F texture")
    if quality not in (GPUX_BC6H_OneRegion, GPUX_BC6H_TwoRegions):
        raise ValueError("encode_bc6h: quality is GPUX_BC6H_OneRegion or GPUX_BC6H_TwoRegions")
    if quality == GPUX_BC6H_OneRegion:
        raw = _read_back(lambda g, buf: L.GPUX_OpEncodeBC6H(g, tex, mip, buf, 0), nbytes)
    else:
        raw = _read_back(lambda g, buf: L.GPUX_OpEncodeBC6HEx(g, tex, mip, buf, 0, quality), nbytes)
    return np.frombuffer(raw, np.uint8).reshape(-1, 16).copy()


def encode_dds(tex, first_mip=0, mip_count=0, out_format=PBR_DDS_OUT_SAME):
    """PBR_EncodeTextureDDS -> the file's bytes."""
    L = lib()
    size = C.c_size_t(0)
    p = L.PBR_EncodeTextureDDS(tex, first_mip, mip_count, out_format, C.byref(size))
    if not p:
        raise RuntimeError("PBR_EncodeTextureDDS failed")
    try:
        return C.string_at(p, size.value)
    finally:
        _libc_free(p)


def _libc_free(p):
    libc = C.CDLL(None)
    libc.free.argtypes = [VP]
    libc.free.restype = None
    libc.free(p)


def write_dds(path, tex, first_mip=0, mip_count=0, out_format=PBR_DDS_OUT_SAME):
    if lib().PBR_WriteTextureDDS(os.fsencode(path), tex, first_mip, mip_count, out_format) != 0:
        raise RuntimeError("PBR_WriteTextureDDS failed")


def make_texture_from_float_dds_file(path):
    t = lib().PBR_MakeTextureFromFloatDDSFile(os.fsencode(path))
    if not t:
        raise RuntimeError("PBR_MakeTextureFromFloatDDSFile failed")
    return t


def decode_bc6h(blocks, w, h, layers, fmt):
    """BC6H_UF16 blocks of one level (uint8 [layers * bh * bw][16], layer after layer) decoded by K19 through GPUX_OpDecodeBC6H into a
    fresh `fmt` (Format_RGBA32F / Format_RGBA16F) texture -> the level as read_mip gives it, always [layers][h][w][4]."""
    L = lib()
    blocks = np.ascontiguousarray(blocks, np.uint8)
    if layers not in (1, 6) or blocks.size != ((w + 3) // 4) * ((h + 3) // 4) * 16 * layers:
        raise ValueError("decode_bc6h: one 2-D level or six cube faces of ceil(w/4) x ceil(h/4) blocks each")
    tex = make_texture(fmt, w, h, TextureFlag_Cubemap if layers == 6 else 0)
    buf = L.GPU_MakeBuffer(blocks.size, BufferFlag_CPU, blocks.ctypes.data_as(VP))
    g = L.GPU_MakeGraph()
    try:
        L.GPUX_OpDecodeBC6H(g, buf, 0, tex, 0)
        L.GPU_GraphSubmit(g)
        L.GPU_GraphWait(g)
        out = read_mip(tex, 0)
    finally:
        L.GPU_DestroyGraph(g)
        L.GPU_DestroyBuffer(buf)
        L.GPU_DestroyTexture(tex)
    return out if layers > 1 else out[None]


def make_texture_from_bc6h_dds_file(path, fmt):
    t = lib().PBR_MakeTextureFromBC6HDDSFile(os.fsencode(path), fmt)
    if not t:
        raise RuntimeError("PBR_MakeTextureFromBC6HDDSFile failed")
    return t


def decode_bc6h_blocks_host(blocks, w, h):
    """PBR_DecodeBC6HBlocks: the contract's arithmetic on the host -> half bits uint16 [h][w][3]."""
    blocks = np.ascontiguousarray(blocks, np.uint8)
    assert blocks.size == ((w + 3) // 4) * ((h + 3) // 4) * 16
    out = np.zeros((h, w, 3), np.uint16)
    lib().PBR_DecodeBC6HBlocks(blocks.ctypes.data_as(VP), w, h, out.ctypes.data_as(C.POINTER(C.c_uint16)))
    return out


def panorama_directions(w, h):
    """GPUX_PanoramaDirections: the fp32 directions K20 samples along -> float32 [h][w][3] (host code, needs no GPU)."""
    out = np.zeros((int(h), int(w), 3), np.float32)
    if int(w) < 1 or int(h) < 1 or lib().GPUX_PanoramaDirections(int(w), int(h), out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise ValueError("panorama_directions: extents are 1 .. 16384")
    return out


def cube_to_panorama(cube, mip=0, width=0, height=0, fmt=Format_RGBA32F):
    """Level `mip` of an RGBA32F cube as a lat-long panorama (K20 through PBR_MakePanoramaFromCube; width 0: 4 n, height 0: width / 2)
    -> float32 [h][w][4], or for fmt=Format_RGBA16F the half bit patterns as uint16 [h][w][4]."""
    L = lib()
    pano = L.PBR_MakePanoramaFromCube(cube, mip, width, height, fmt)
    if not pano:
        raise RuntimeError("PBR_MakePanoramaFromCube failed")
    try:
        out = read_mip(pano, 0)
    finally:
        L.GPU_DestroyTexture(pano)
    return out.view(np.uint16) if fmt == Format_RGBA16F else out


def prefilter_ggx_samples(roughness, samples, src_size, src_levels, lod_bias=1.0):
    """GPUX_PrefilterGGXSamples: the table K21 uses -> (float32 [kept][4] of {l.x, l.y, l.z, lod}, wsum as np.float32); host code,
    needs no GPU"""
    n = int(samples)
    out = np.zeros((max(n, 1), 4), np.float32)
    kept, wsum = U32(0), C.c_float(0.0)
    if n < 1 or n > 4096 or lib().GPUX_PrefilterGGXSamples(float(roughness), n, int(src_size), int(src_levels), float(lod_bias),
                                                          out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(kept), C.byref(wsum)) != 0:
        raise ValueError("prefilter_ggx_samples: bad arguments")
    return out[:kept.value].copy(), np.float32(wsum.value)


def prefilter_ggx(env, dst, mip, roughness, samples, lod_bias=1.0, faces=(0, 6), rows=None):
    """Level `mip` of the RGBA32F cube `dst` from the RGBA32F cube `env` by K21 (GPUX_OpPrefilterGGX in a graph of its own, blocking);
    rows=None: the whole level."""
    L = lib()
    if rows is None:
        rows = (0, max(1, dst.contents.width >> mip))
    g = L.GPU_MakeGraph()
    try:
        L.GPUX_OpPrefilterGGX(g, env, dst, mip, float(roughness), int(samples), float(lod_bias), int(faces[0]), int(faces[1]), int(rows[0]), int(rows[1]))
        L.GPU_GraphSubmit(g)
        L.GPU_GraphWait(g)
    finally:
        L.GPU_DestroyGraph(g)


BrdfLut_SmithSchlick, BrdfLut_SmithCorrelated = 0, 1


def brdf_lut_ggx_samples(count):
    """GPUX_BrdfLutGGXSamples: the table K22 uses -> float32 [count][3] of {xi1, cos phi, sin phi}; host code, needs no GPU"""
    n = int(count)
    out = np.zeros((max(n, 1), 3), np.float32)
    if n < 1 or n > 4096 or lib().GPUX_BrdfLutGGXSamples(n, out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise ValueError("brdf_lut_ggx_samples: bad arguments")
    return out


def brdf_lut_ggx(tex, count, visibility=0, rows=None):
    """Rows `rows` of the 2-D texture `tex` as the GGX split-sum LUT by K22 (GPUX_OpBrdfLutGGX in a graph of its own, blocking);
    rows=None: the whole map."""
    L = lib()
    if rows is None:
        rows = (0, tex.contents.height)
    g = L.GPU_MakeGraph()
    try:
        L.GPUX_OpBrdfLutGGX(g, tex, int(count), int(visibility), int(rows[0]), int(rows[1]))
        L.GPU_GraphSubmit(g)
        L.GPU_GraphWait(g)
    finally:
        L.GPU_DestroyGraph(g)
