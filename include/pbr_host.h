/*
 * pbr_host.h -- C host layer above the GPU_* boundary: the reference renderer's own call
 * sequences for the IBL precompute and the lighting pass, restated in C11 against gpu_hip.h so
 * that they run headless (no window, no assimp, no glslang).  Every function cites the reference
 * code whose GPU_* call sequence it reproduces; a reference maintainer could delete these and
 * keep calling GPU_* from render.cpp unchanged.
 */
#ifndef PBR_HOST_H
#define PBR_HOST_H

#include "gpux.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- A1: Radiance .hdr (RGBE) decode, what stbi_loadf(..., 4) returns for asset_import.cpp:19
 * (third_party/stb_image.h:7130-7286): flat or new-RLE scanlines, rgb = mantissa * 2^(e-136),
 * alpha = 1, e == 0 -> 0.  Returns malloc'ed float RGBA [h][w][4] or NULL (reason in *err). */
float* PBR_DecodeHDR(const void* bytes, size_t size, int* w, int* h, const char** err);

/* asset_import.cpp:17-27: vertical strip of 6 square faces (height == 6*width) -> RGBA32F cubemap
 * with a full mip chain (GPU_MakeTexture uploads and generates the mips before returning). */
GPU_Texture* PBR_MakeTextureFromHDRIMemory(const void* bytes, size_t size);
GPU_Texture* PBR_MakeTextureFromHDRIFile(const char* filepath);

/* ---- extensions around the input/output files ----
 * Equirectangular .hdr (2:1) -> cubemap with mips; the strip loader above stays the reference path. */
GPU_Texture* PBR_MakeTextureFromEquirectHDRIMemory(const void* bytes, size_t size, uint32_t face_size);
GPU_Texture* PBR_MakeTextureFromEquirectHDRIFile(const char* filepath, uint32_t face_size);
/* Radiance RGBE writer (flat scanlines): returns malloc'ed file bytes, *out_size set. rgba: float [h][w][4] (alpha dropped). */
void* PBR_EncodeHDR(const float* rgba, int w, int h, size_t* out_size);
int   PBR_WriteHDRFile(const char* filepath, const float* rgba, int w, int h);
/* One mip of a cubemap as a vertical-strip .hdr (the layout MakeTextureFromHDRIFile reads back). Returns 0 on success. */
int   PBR_WriteCubeStripHDR(const char* filepath, GPU_Texture* cube, uint32_t mip_level);
/* One level of an RGBA32F cubemap as a lat-long panorama (K20, GPUX_OpCubeToPanorama: Z-up, row 0 next to +Z, the inverse of the
 * equirectangular loader above; host/pbr_panorama.c): a new 2-D texture of `format` (GPU_Format_RGBA32F or GPU_Format_RGBA16F) that the
 * caller destroys.  width 0 means 4 n and height 0 means width / 2 (at least 1), n the level's face size; either may be anything from 1
 * to 16384.  Blocking (own graph).  NULL on any error.  The level is the caller's choice and is sampled bilinearly with no minification
 * filter: on the specular map the levels are roughness levels, not a filter chain, so a width far below 4 n aliases instead of moving
 * to a smaller level.  A panorama as .dds, BC6H included, needs nothing more: it is PBR_WriteTextureDDS of the texture returned. */
GPU_Texture* PBR_MakePanoramaFromCube(GPU_Texture* cube, uint32_t mip_level, uint32_t width, uint32_t height, GPU_Format format);
/* The RGBA32F panorama of PBR_MakePanoramaFromCube, read back and written with PBR_WriteHDRFile (RGBE).  Returns 0 on success. */
int   PBR_WritePanoramaHDR(const char* filepath, GPU_Texture* cube, uint32_t mip_level, uint32_t width, uint32_t height);

/* ---- IBL precompute, render.cpp:505-619 ---- */
typedef struct PBR_IBLMaps {
    GPU_Texture* irradiance_map;        /* RGBA32F cube, render.cpp:794 (32x32) */
    GPU_Texture* brdf_lut;              /* RG16F 2D,    render.cpp:795 (256x256) */
    GPU_Texture* tex_specular_env_map;  /* RGBA32F cube + mips, render.cpp:796 (256x256) */
} PBR_IBLMaps;

/* render.cpp:794-796 with the sizes as parameters (reference: 32, 256, 256) */
void PBR_MakeIBLMaps(PBR_IBLMaps* maps, uint32_t irradiance_size, uint32_t lut_size, uint32_t specular_size);
void PBR_DestroyIBLMaps(PBR_IBLMaps* maps);

/* One work unit of the precompute = rows [row0,row1) of faces [face0,face1) of one output level. */
typedef enum PBR_UnitKind { PBR_Unit_Prefilter = 0, PBR_Unit_Irradiance = 1, PBR_Unit_BrdfLut = 2 } PBR_UnitKind;
typedef struct PBR_WorkUnit {
    uint32_t kind;                      /* PBR_UnitKind */
    uint32_t mip;                       /* prefilter output mip */
    uint32_t face0, face1, row0, row1;
    double   cost;                      /* texels * samples-per-texel (1 for the copy mip) */
} PBR_WorkUnit;

void PBR_GenIrradianceMap(GPU_Texture* tex_env_cube, GPU_Texture* irradiance_map);           /* render.cpp:505-540 */
/* render.cpp:542-589; min_size = 16 reproduces the reference's `if (size < 16) break;`, 1 runs the whole chain */
void PBR_GenPrefilteredEnvMap(GPU_Texture* tex_env_cube, GPU_Texture* tex_specular_env_map, uint32_t min_size);
/* The same map baked the way the lighting pass reads it (K21, GPUX_OpPrefilterGGX; no reference counterpart): level 0 is the same
 * copy, recorded the same way; level i >= 1 down to min_size is the GGX importance-sampled prefilter of the environment at roughness
 * min(1, i / 4) -- lighting_pass.glsl:699 fetches lod = roughness * 4 -- with sample_count (1 .. 4096) samples per texel and lod bias 1,
 * one op per whole level, all in one graph.  Blocking.  Its split-sum partner is the LUT of PBR_GenBRDFIntegrationMapGGX (K22); PBR_GenBRDFIntegrationMap is K1's Beckmann LUT. */
void PBR_GenPrefilteredEnvMapGGX(GPU_Texture* tex_env_cube, GPU_Texture* tex_specular_env_map, uint32_t min_size, uint32_t sample_count);
void PBR_GenBRDFIntegrationMap(GPU_Texture* brdf_lut);                                       /* render.cpp:591-619 */
/* The split-sum LUT of the GGX lobe by importance sampling (K22, GPUX_OpBrdfLutGGX; no reference counterpart): the partner of
 * PBR_GenPrefilteredEnvMapGGX's map, sample_count (1 .. 4096) samples per texel, visibility a GPUX_BrdfLutVisibility
 * (GPUX_BrdfLut_SmithSchlick is the term lighting_pass.glsl:56-61 evaluates).  Any 2-D RG16F / RG32F / RGBA32F texture up to 4096 a
 * side; one op over all rows.  Blocking. */
void PBR_GenBRDFIntegrationMapGGX(GPU_Texture* brdf_lut, uint32_t sample_count, uint32_t visibility);

/* ---- K17 (no reference counterpart): the nine-coefficient spherical-harmonic form of the environment's diffuse
 * lighting -- the 27 numbers other IBL bakers emit and engines consume in place of an irradiance cube.  Contract (csrc/sh_core.h):
 * coef[3 k + c] = sum over ALL texels of the level of L_c Y_k(d) domega with the exact texel solid angle, fp64; real basis without
 * Condon-Shortley phase in the order 1, y, z, x, xy, yz, 3zz-1, xz, xx-yy; irradiance in the reference's E / (2 pi) normalisation
 * (a constant environment c gives c / 2), NOT clamped: under a strong sun the series rings and may go negative.
 * PBR_GenIrradianceMap (K3: 1024 samples of LOD 6) stays the reference path and the default everywhere. ---- */
int  PBR_ProjectSH9(GPU_Texture* cube, uint32_t mip_level, double out[27]);     /* blocking (own graph + mapped buffer); 0 on success */
/* project level src_mip_level and write mip 0 of irradiance_map from it; PBR_MakeLightingPass* binds the result unchanged */
void PBR_GenIrradianceMapSH(GPU_Texture* tex_env_cube, uint32_t src_mip_level, GPU_Texture* irradiance_map);
void PBR_EvalSH9Irradiance(const double coef[27], const float n[3], float rgb[3]);   /* host, the same contract; n is normalised in double */
/* text: one '#' line naming basis order and convention, then 9 lines of 3 values (%.17g: the bits survive).  0 on success; the
 * reader refuses anything else (a missing or truncated line, a token that is not a number, trailing text). */
int  PBR_WriteSH9File(const char* path, const double coef[27]);
int  PBR_ReadSH9File(const char* path, double coef[27]);
/* Records (does not submit) the dispatches of an explicit unit list into `graph`: the sharded form of the above.
 * `arena` receives the per-unit descriptor sets (caller resets it after GPU_GraphWait). */
typedef struct PBR_IBLPipelines PBR_IBLPipelines;
PBR_IBLPipelines* PBR_MakeIBLPipelines(void);
void PBR_DestroyIBLPipelines(PBR_IBLPipelines* p);
void PBR_RecordUnits(PBR_IBLPipelines* p, GPU_Graph* graph, GPU_DescriptorArena* arena, GPU_Texture* tex_env_cube,
                     const PBR_IBLMaps* maps, const PBR_WorkUnit* units, uint32_t unit_count);
/* One level of PBR_GenPrefilteredEnvMap's graph: the descriptor set from `arena`, the prefilter pipeline, the level as push constant and
 * the reference's size / 8 dispatch.  For host code that records the bake's levels itself (PBR_GenPrefilteredEnvMapGGX). */
void PBR_RecordPrefilterLevel(PBR_IBLPipelines* p, GPU_Graph* graph, GPU_DescriptorArena* arena, GPU_Texture* tex_env_cube,
                              GPU_Texture* tex_specular_env_map, uint32_t mip_level);

/* Splits the precompute (prefilter mips down to min_size, optionally irradiance) over `world` ranks: the rows of
 * the big levels, laid end to end and weighted with the measured time per sample evaluation of their level, are cut into
 * `world` contiguous shares of equal cost, so a rank receives at most two partial faces plus runs of whole faces (one unit per
 * run); the copy level is pinned to rank 0 (where results are gathered), cheap levels stay whole.  world = 1: one unit per level.
 * Returns the number of units written to out (<= capacity) for `rank`; rank < 0 lists all units.  Deterministic. */
uint32_t PBR_PartitionIBL(uint32_t specular_size, uint32_t min_size, uint32_t irradiance_size, uint32_t env_size,
                          int world, int rank, PBR_WorkUnit* out, uint32_t capacity);

/* ---- the exchange step of the multi-GPU job: RCCL over xGMI, one grouped batch of point-to-point transfers.
 * The reference has no counterpart (single queue, gpu_vulkan.c:1040-1106).  `nccl_comm` is the caller's ncclComm_t (opaque:
 * the library does not own the bootstrap), `stream` the hipStream_t the transfers are enqueued on -- pass
 * GPUX_GraphStream(graph) after GPU_GraphSubmit(graph) and the exchange follows the graph's kernels without a host round
 * trip; GPU_GraphWait(graph) then also waits for the exchange.  Negative return values are PBR_E_*. ---- */
enum { PBR_OK = 0, PBR_E_BADARG = -1, PBR_E_COMM = -2 };
typedef struct PBR_XferRange { void* ptr; uint64_t bytes; int peer; } PBR_XferRange;    /* device pointer, byte count, peer rank */
/* RCCL is bound at first use (dlopen), never at link time: libgpu_hip.so has no librccl dependency, and the exchange calls the
 * copy of librccl the process already holds -- the one that made `nccl_comm`.  Search order: PBR_SetRcclLibrary(path) or
 * env PBR_RCCL_LIB; an already mapped "librccl.so.1"; the process's global symbols; a fresh dlopen of librccl.so.1.
 * PBR_SetRcclLibrary(NULL) forgets the binding (next use searches again).  PBR_RcclInfo: ncclGetVersion() code (e.g. 22707) and
 * the file the entry points were bound from.  PBR_CommInfo: ncclCommCount / ncclCommUserRank of the caller's communicator. */
int PBR_SetRcclLibrary(const char* path);
int PBR_RcclInfo(int* version, const char** path);
int PBR_CommInfo(void* nccl_comm, int* count, int* user_rank);
/* ncclGroupStart; ncclRecv x n_recvs; ncclSend x n_sends; ncclGroupEnd (a rank may send to itself).  If a call inside the group
 * fails, the group is still closed before PBR_E_COMM is returned (no dangling group on this thread); the communicator must then
 * be treated as dead. */
int PBR_ExchangeRanges(void* nccl_comm, void* stream, const PBR_XferRange* sends, uint32_t n_sends,
                       const PBR_XferRange* recvs, uint32_t n_recvs);
/* The bytes of one work unit inside its texture: contiguous in the [mip][face][y][x] layout (rows of one face, or whole faces). */
int PBR_UnitByteRange(const PBR_IBLMaps* maps, const PBR_WorkUnit* unit, GPU_Texture** texture, uint64_t* offset, uint64_t* bytes);
/* After every rank has run its share (PBR_PartitionIBL(..., world, rank) + PBR_RecordUnits): ranks != root send their units,
 * root receives all of them in place, so that `maps` on root holds the whole result.  Every rank must pass the same
 * min_size / env_size it partitioned with.  Returns the bytes this rank sent or received (0 when world == 1). */
int64_t PBR_GatherUnits(void* nccl_comm, void* stream, int root, int world, int rank, const PBR_IBLMaps* maps,
                        uint32_t min_size, uint32_t env_size);
/* The same for a subset of the levels: bit l of level_mask = prefilter mip l, PBR_LEVEL_IRRADIANCE = the irradiance map.
 * All ranks must call the phases in the same order (one communicator: RCCL keeps issue order). */
#define PBR_LEVEL_IRRADIANCE 0x80000000u
int64_t PBR_GatherUnitsMasked(void* nccl_comm, void* stream, int root, int world, int rank, const PBR_IBLMaps* maps,
                              uint32_t min_size, uint32_t env_size, uint32_t level_mask);
/* The transfers PBR_GatherUnitsMasked would enqueue for `rank` (root: receives from every peer; others: sends to root), without
 * a communicator: out may be NULL to count.  Returns the number of ranges. */
int64_t PBR_GatherPlan(int root, int world, int rank, const PBR_IBLMaps* maps, uint32_t min_size, uint32_t env_size,
                       uint32_t level_mask, PBR_XferRange* out, uint32_t capacity);
/* units[i] whose level is in level_mask, in order; out may alias nothing; returns the count */
uint32_t PBR_SelectUnits(const PBR_WorkUnit* units, uint32_t n, uint32_t level_mask, PBR_WorkUnit* out);
/* One rank's whole share with the exchange overlapped: the units of `early_mask` (the level that is most bytes on the wire: mip 1,
 * i.e. early_mask = 2) are recorded into g_early behind whatever the caller already recorded there (the source's
 * GPU_OpGenerateMipmaps), the rest into g_late; both are submitted, then the early units travel on g_early's stream while
 * g_late computes, the late ones follow g_late.  The caller waits: GPU_GraphWait(g_late); GPU_GraphWait(g_early); and resets
 * the arena.  world == 1 runs both graphs and moves nothing.  Returns bytes sent / received by this rank, or PBR_E_*.
 * After a NEGATIVE return both graphs are nevertheless submitted: the caller must still GPU_GraphWait both, and must treat the
 * communicator as dead (a failed early exchange means the late one was never issued; peers may be waiting in theirs). */
int64_t PBR_RunPartitionedIBL(PBR_IBLPipelines* p, GPU_Graph* g_early, GPU_Graph* g_late, GPU_DescriptorArena* arena,
                              GPU_Texture* tex_env_cube, const PBR_IBLMaps* maps, void* nccl_comm, int root, int world, int rank,
                              uint32_t min_size, uint32_t early_mask);
/* Screen-band split of the shade pass (C5): rank r owns rows [height*r/world, height*(r+1)/world) of the frame */
void PBR_BandRows(uint32_t height, int world, int rank, uint32_t* row0, uint32_t* row1);
int64_t PBR_GatherBands(void* nccl_comm, void* stream, int root, int world, int rank, GPU_Texture* frame);

/* ---- camera + Globals: utils/camera.h:95-120 and render.cpp:962-991 ---- */
typedef struct PBR_Globals {            /* RendererGlobalsBuffer, render.h:122-136; column-major mat4 */
    float clip_space_from_world[16];
    float clip_space_from_view[16];
    float world_space_from_clip[16];
    float view_space_from_clip[16];
    float view_space_from_world[16];
    float world_space_from_view[16];
    float sun_space_from_world[16];
    float old_clip_space_from_world[16];
    float sun_direction[4];
    float camera_pos[3];
    float frame_idx_mod_59;
    float lightgrid_scale;
    /* != 0: the lighting pass draws the light-grid visualiser instead of the shaded frame (lighting_pass.glsl:463-491, the reference's G
     * key: main.cpp:79, render.cpp:990) -- kernel K16 over the recorded rows, whatever the pipeline's shade flags; needs LIGHTGRID bound
     * (PBR_MakeLightingPassLive).  PBR_FillGlobals writes 0; there is no entry point of its own: set the field after PBR_FillGlobals. */
    uint32_t visualize_lightgrid;
} PBR_Globals;

/* ori_xyzw == NULL -> the reference's default orientation (faces +Y, utils/camera.h:45). */
void PBR_FillGlobals(PBR_Globals* out, const float pos[3], const float ori_xyzw[4], float fov_degrees, float aspect,
                     float z_near, float z_far, float sun_angle_x_deg, float sun_angle_y_deg, uint32_t frame_idx);

/* ---- lighting pass: layout/descriptor set of render.cpp:829-871, pass of :716-723, draw of :1119-1127 ---- */
typedef struct PBR_GBuffer {
    GPU_Texture* base_color; GPU_Texture* normal; GPU_Texture* orm; GPU_Texture* emissive; GPU_Texture* depth;   /* render.cpp:680-687 */
    GPU_Texture* lighting_result;                                                                                /* render.cpp:693 */
} PBR_GBuffer;
void PBR_MakeGBuffer(PBR_GBuffer* gb, uint32_t width, uint32_t height, GPU_Format result_format);
void PBR_DestroyGBuffer(PBR_GBuffer* gb);

typedef struct PBR_LightingPass PBR_LightingPass;
PBR_LightingPass* PBR_MakeLightingPass(const PBR_GBuffer* gb, const PBR_IBLMaps* maps, uint32_t width, uint32_t height);
/* the same with the sun depth map of the shadow pass bound to SUN_DEPTH_MAP (render.cpp:676, :863; D32F); NULL = 1x1 stand-in.
 * GPUX_SetShadeFlags(PBR_LightingPipeline(lp), ... | GPUX_Shade_SunShadows) makes the pass read it. */
PBR_LightingPass* PBR_MakeLightingPassEx(const PBR_GBuffer* gb, const PBR_IBLMaps* maps, uint32_t width, uint32_t height, GPU_Texture* sun_depth_map);
/* all raster-fed inputs of the live shader (render.cpp:861-863): the swept light grid (PBR_LightgridTexture), the previous frame
 * as the lighting pass sees it (the reference binds bloom_downscale_rt: PBR_PostBloomDownscale) and the sun depth map; NULLs = stand-ins.
 * GPUX_Shade_LightShafts | GPUX_Shade_SunShadows | GPUX_Shade_VoxelGI then runs the reference's complete live shader. */
PBR_LightingPass* PBR_MakeLightingPassLive(const PBR_GBuffer* gb, const PBR_IBLMaps* maps, uint32_t width, uint32_t height,
                                           GPU_Texture* sun_depth_map, GPU_Texture* lightgrid, GPU_Texture* prev_frame_result);
void PBR_DestroyLightingPass(PBR_LightingPass* lp);
GPU_Buffer* PBR_LightingGlobalsBuffer(PBR_LightingPass* lp);           /* persistently mapped (render.cpp:675) */
GPU_GraphicsPipeline* PBR_LightingPipeline(PBR_LightingPass* lp);
/* Ambient term from SH9 coefficients in place of the irradiance cube (K5 with GPUX_Shade_SH9Irradiance): 27 doubles at `offset` (a
 * multiple of 8) of `coef`, as GPUX_OpProjectSH9 writes them; they are read on the device when a recorded pass executes.  Sets the
 * flag and the buffer on the pass's pipeline for the passes recorded from now on; NULL restores the cube path.  A pass made from maps
 * whose irradiance_map is NULL can only be drawn this way.  (GPUX_SetShadeFlags replaces all flags: call it before this.) */
void PBR_LightingUseSH9(PBR_LightingPass* lp, GPU_Buffer* coef, uint32_t offset);
/* render.cpp:977-991 + 1119-1127: copies globals into the mapped buffer and records the pass; rows [row0,row1), row1 == 0 -> all */
void PBR_RecordLightingPass(PBR_LightingPass* lp, GPU_Graph* graph, const PBR_Globals* globals, uint32_t row0, uint32_t row1);

/* ---- voxel light grid + its sweep pass: render.cpp:678 (image), :816 (IMG0 binding), :151-187 (pipeline,
 *      descriptor set), :1028 (clear), :1061-1072 (per-frame sweep) ---- */
typedef struct PBR_Lightgrid PBR_Lightgrid;
PBR_Lightgrid* PBR_MakeLightgrid(uint32_t size);                 /* reference: LIGHTGRID_SIZE 128 (render.cpp:7); size >= 128, multiple of 8 */
void PBR_DestroyLightgrid(PBR_Lightgrid* lg);
GPU_Texture* PBR_LightgridTexture(PBR_Lightgrid* lg);
uint32_t PBR_LightgridSweepDirection(const PBR_Lightgrid* lg);   /* direction used by the last recorded sweep */
void PBR_RecordLightgridClear(PBR_Lightgrid* lg, GPU_Graph* graph);
/* advances the direction (1, 2, 0, 1, ... from a fresh grid, as render.cpp:1064-1065) and records the full dispatch */
void PBR_RecordLightgridSweep(PBR_Lightgrid* lg, GPU_Graph* graph);
/* sharded form: invocations (iy, iz) in [y0,y1) x [z0,z1) of an explicit direction; lines are independent */
void PBR_RecordLightgridSweepLines(PBR_Lightgrid* lg, GPU_Graph* graph, uint32_t direction, uint32_t y0, uint32_t y1, uint32_t z0, uint32_t z1);

/* ---- post-process tail: TAA resolve (render.cpp:281-337, 690-697, 732-739, 1131-1137) and the final
 *      tone-map pass (render.cpp:456-501, 782-785, 1181-1187).  frame_idx selects the ping-pong half exactly as
 *      frame_idx_mod2 does in the reference: frame i resolves into taa_output_rt[i%2] reading taa_output_rt[1-i%2]. ---- */
typedef struct PBR_PostProcess PBR_PostProcess;
/* gb supplies GBUFFER_DEPTH and LIGHTING_RESULT (RGBA16F); backbuffer_format stands in for the swapchain (RGBA8UN / BGRA8UN, or a float format) */
PBR_PostProcess* PBR_MakePostProcess(const PBR_GBuffer* gb, uint32_t width, uint32_t height, GPU_Format backbuffer_format);
void PBR_DestroyPostProcess(PBR_PostProcess* pp);
GPU_Texture* PBR_PostVelocity(PBR_PostProcess* pp, uint32_t frame_idx_mod2);     /* gbuffer_velocity[i]: RG16F, uploaded by the caller */
GPU_Texture* PBR_PostTaaOutput(PBR_PostProcess* pp, uint32_t frame_idx_mod2);    /* taa_output_rt[i] */
GPU_Texture* PBR_PostBackbuffer(PBR_PostProcess* pp);
void PBR_RecordTaaResolve(PBR_PostProcess* pp, GPU_Graph* graph, uint32_t frame_idx);
void PBR_RecordTaaResolveRows(PBR_PostProcess* pp, GPU_Graph* graph, uint32_t frame_idx, uint32_t row0, uint32_t row1);   /* rows [row0,row1) only */
void PBR_RecordFinalPostProcess(PBR_PostProcess* pp, GPU_Graph* graph, uint32_t frame_idx);
/* bloom chain between the two (render.cpp:741-777, 340-454, 1139-1176): BLOOM_PASS_COUNT (6, or fewer on tiny frames) 13-tap
 * downsamples into the mips of a half-size target, clear + blit of the TAA result into the full-size target, as many additive
 * tent upsamples; then the final pass reading that target, as the reference binds it (render.cpp:478). */
void PBR_RecordBloom(PBR_PostProcess* pp, GPU_Graph* graph, uint32_t frame_idx);
void PBR_RecordFinalPostProcessBloom(PBR_PostProcess* pp, GPU_Graph* graph, uint32_t frame_idx);
GPU_Texture* PBR_PostBloomDownscale(PBR_PostProcess* pp);
GPU_Texture* PBR_PostBloomUpscale(PBR_PostProcess* pp);
uint32_t PBR_PostBloomPassCount(const PBR_PostProcess* pp);

/* ---- sun shadow depth pass (N5 / K12): render.cpp:88-111 (pipeline), :677 + :725-729 (2048^2 D32F target and its depth-only
 *      render pass), :995-1020 (per-frame clear + one indexed draw per part); asset_import.cpp:172-173 (merged buffers) ---- */
typedef struct PBR_MeshPart { uint32_t first_index, index_count; } PBR_MeshPart;     /* RenderObjectPart's draw range */
typedef struct PBR_Mesh PBR_Mesh;
/* vertices: vertex_count x 11 floats (render.h:31-36 Vertex: position, normal, tangent, tex_coord); 32-bit indices */
PBR_Mesh* PBR_MakeMesh(const float* vertices_11f, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count,
                       const PBR_MeshPart* parts, uint32_t part_count);
void PBR_DestroyMesh(PBR_Mesh* mesh);
GPU_Buffer* PBR_MeshVertexBuffer(PBR_Mesh* mesh);
GPU_Buffer* PBR_MeshIndexBuffer(PBR_Mesh* mesh);
uint32_t PBR_MeshPartCount(const PBR_Mesh* mesh);

typedef struct PBR_SunDepthPass PBR_SunDepthPass;
PBR_SunDepthPass* PBR_MakeSunDepthPass(uint32_t size);                 /* reference: 2048 */
void PBR_DestroySunDepthPass(PBR_SunDepthPass* pass);
GPU_Texture* PBR_SunDepthTexture(PBR_SunDepthPass* pass);              /* D32F size^2: bind it as SUN_DEPTH_MAP (PBR_MakeLightingPassLive) */
GPU_Buffer* PBR_SunDepthGlobalsBuffer(PBR_SunDepthPass* pass);         /* persistently mapped PBR_Globals */
GPU_GraphicsPipeline* PBR_SunDepthPipeline(PBR_SunDepthPass* pass);
GPU_RenderPass* PBR_SunDepthRenderPass(PBR_SunDepthPass* pass);
GPU_PipelineLayout* PBR_SunDepthLayout(PBR_SunDepthPass* pass);        /* one buffer binding, "GLOBALS" */
GPU_DescriptorSet* PBR_SunDepthDescriptorSet(PBR_SunDepthPass* pass);
/* render.cpp:991 + 995-1020: copies globals (if not NULL) into the mapped buffer, clears the map to 1 and draws every part */
void PBR_RecordSunDepthPass(PBR_SunDepthPass* pass, GPU_Graph* graph, const PBR_Mesh* mesh, const PBR_Globals* globals);

/* ---- geometry pass (K13): render.cpp:190-233 (pipelines), :680-708 (targets, render passes), :993 + :1076-1115 (per-frame clear
 *      and one indexed draw per part, then the skybox with its own buffers); a part's material = its four RGBA8UN textures ---- */
typedef struct PBR_Material PBR_Material;
/* four size x size RGBA8 level-0 images (base colour, normal, ORM, emissive); size a power of two; mips are generated */
PBR_Material* PBR_MakeMaterial(uint32_t size, const void* base_color, const void* normal, const void* orm, const void* emissive);
void PBR_DestroyMaterial(PBR_Material* material);
GPU_Texture* PBR_MaterialTexture(PBR_Material* material, uint32_t which);    /* 0 .. 3 in the order above */
void PBR_MeshSetPartMaterial(PBR_Mesh* mesh, uint32_t part, PBR_Material* material);   /* the material is not owned by the mesh */
/* a material over textures the caller made (2-D RGBA8UN, BC1, BC3 or BC5; e.g. PBR_MakeTextureFromDDSFile) and keeps owning: they
 * must outlive the material.  A NULL slot gets the 1 x 1 dummy of render.cpp:787-793 (white, flat normal, black, black), owned by
 * the material. */
PBR_Material* PBR_MakeMaterialFromTextures(GPU_Texture* const tex[4]);

/* ---- .dds material textures (N8 / K15; the parser in host/pbr_dds.c, the loaders in host/pbr_ddsin.c): what asset_import.cpp:30-60
 *      (LoadMeshTexture, through ddspp) accepts ---- */
enum { PBR_DDS_MAX_LEVELS = 16 };
typedef struct PBR_DDSInfo {
    GPU_Format format;            /* BC1_RGBA_UN (DXT1, DXGI 71), BC3_RGBA_UN (DXT5, 77), BC5_UN (ATI2 / BC5U, 83), RGBA8UN (DXGI 28, R G B A byte masks) */
    uint32_t width, height;
    uint32_t level_count;         /* 1 .. PBR_DDS_MAX_LEVELS */
    uint64_t level_offset[PBR_DDS_MAX_LEVELS], level_size[PBR_DDS_MAX_LEVELS];   /* bytes from the start of the file; inside it */
} PBR_DDSInfo;
/* 0 and *out filled, or a negative PBR_DDS_E_* (PBR_DDSErrorString names it): not a DDS, a truncated header or payload, a level
 * count the file (or a full chain) cannot hold, a cube / volume / array file, extents of 0 or above 16384, any other pixel format */
enum { PBR_DDS_E_ARG = -1, PBR_DDS_E_MAGIC = -2, PBR_DDS_E_TRUNCATED = -3, PBR_DDS_E_FORMAT = -4, PBR_DDS_E_LAYOUT = -5, PBR_DDS_E_EXTENT = -6,
       PBR_DDS_E_LEVELS = -7 };
int PBR_ParseDDS(const void* bytes, size_t size, PBR_DDSInfo* out);
const char* PBR_DDSErrorString(int code);
enum { PBR_DDS_FILE_MIPS = 1 };   /* also upload the file's levels below 0, down to the count GPU_TextureFlag_HasMipmaps gives */
/* flags == 0: GPU_MakeTexture(format, w, h, 1, 0, level 0), the reference's behaviour.  With PBR_DDS_FILE_MIPS a file of one level
 * still gives a one-level texture; a file of several must hold every level of the chain.  NULL on any error (message on stderr). */
GPU_Texture* PBR_MakeTextureFromDDSMemory(const void* bytes, size_t size, uint32_t flags);
GPU_Texture* PBR_MakeTextureFromDDSFile(const char* filepath, uint32_t flags);

/* ---- the bake's maps as .dds files (N11 / K18; the container in host/pbr_dds.c, the writer in host/pbr_ddsout.c, the float loader in
 *      host/pbr_ddsin.c): one DX10-header container per texture with its mip chain; cubes
 *      carry the TEXTURECUBE flag and all six faces, data face-major (+X -X +Y -Y +Z -Z, the layer order), each face's levels in order. ---- */
typedef struct PBR_DDSInfoEx {
    uint32_t dxgi_format;         /* 2 RGBA32F, 10 RGBA16F, 34 RG16F, 95 BC6H_UF16, 28 RGBA8UN, 71 BC1, 77 BC3, 83 BC5 (legacy FourCCs map to these) */
    uint32_t width, height;
    uint32_t layers;              /* 1, or 6 for a cube */
    uint32_t level_count;         /* 1 .. PBR_DDS_MAX_LEVELS */
    uint64_t level_offset[6][PBR_DDS_MAX_LEVELS];   /* [layer][level]: bytes from the start of the file; inside it */
    uint64_t level_size[PBR_DDS_MAX_LEVELS];        /* bytes of one layer of a level */
} PBR_DDSInfoEx;
/* like PBR_ParseDDS (same error codes; that function and what it accepts stay as they are), but also cubes and the float / BC6H formats */
int PBR_ParseDDSEx(const void* bytes, size_t size, PBR_DDSInfoEx* out);
/* the 148 header bytes of such a file and, if layout is not NULL, where every (layer, level) goes; returns the file's size, 0 for
 * arguments that have no DDS form (a format outside the list above, extents of 0 or above 16384, layers not 1 or 6, a non-square cube,
 * more levels than a full chain or than PBR_DDS_MAX_LEVELS).  Host only. */
uint64_t PBR_BuildDDSHeader(uint32_t dxgi_format, uint32_t width, uint32_t height, uint32_t layers, uint32_t level_count, uint8_t header[148],
                            PBR_DDSInfoEx* layout);
enum { PBR_DDS_OUT_SAME = 0,          /* RGBA32F -> DXGI 2, RGBA16F -> DXGI 10, RG16F -> DXGI 34 (the BRDF LUT) */
       PBR_DDS_OUT_RGBA16F = 1,       /* RGBA32F narrowed on the host: round to nearest even, sign and Inf kept (csrc/bc6h_core.h) */
       PBR_DDS_OUT_BC6H_UF16 = 2,     /* RGBA32F / RGBA16F -> DXGI 95 through GPUX_OpEncodeBC6H, every level in one graph */
       PBR_DDS_OUT_BC6H_UF16_2R = 3 };/* the same file with every level encoded at GPUX_BC6H_TwoRegions (csrc/bc6h2_core.h): slower, lower error */
/* levels [first_mip, first_mip + mip_count) of a 2-D or cube texture (mip_count 0: to the end of the chain) as file bytes the caller
 * frees; blocking.  NULL (message on stderr) for a format / output pair outside the list, a bad range or a failed allocation. */
void* PBR_EncodeTextureDDS(GPU_Texture* texture, uint32_t first_mip, uint32_t mip_count, int out_format, size_t* out_size);
int PBR_WriteTextureDDS(const char* path, GPU_Texture* texture, uint32_t first_mip, uint32_t mip_count, int out_format);   /* 0 on success */
/* RGBA32F, RGBA16F and RG16F files, 2-D or cube, with the file's levels: one level gives a texture without mips, several must be the
 * whole chain of GPU_TextureFlag_HasMipmaps.  NULL on any error (message on stderr).  BC6H files are not loaded by this function. */
GPU_Texture* PBR_MakeTextureFromFloatDDSMemory(const void* bytes, size_t size);
GPU_Texture* PBR_MakeTextureFromFloatDDSFile(const char* filepath);
/* BC6H_UF16 files (DXGI 95 as PBR_ParseDDSEx reports it; N12 / K19, host/pbr_ddsin.c), 2-D or cube, any of the format's 14 modes, as an
 * RGBA32F or RGBA16F texture (`target`) the lighting pass takes: every level is decoded once by GPUX_OpDecodeBC6H, all of them in one
 * graph from one staging buffer.  One level gives a texture without mips, several one with GPU_TextureFlag_HasMipmaps; the file may hold
 * fewer levels than the chain (pbr_demo ... dds writes the specular cube down to min_size): the others stay zero, as GPU_MakeTexture
 * leaves them.  NULL on any error (message on stderr). */
GPU_Texture* PBR_MakeTextureFromBC6HDDSMemory(const void* bytes, size_t size, GPU_Format target);
GPU_Texture* PBR_MakeTextureFromBC6HDDSFile(const char* filepath, GPU_Format target);
/* ceil(w / 4) x ceil(h / 4) BC6H_UF16 blocks, row-major -> w x h x 3 half bit patterns (0 .. 0x7BFF), tight rows: the arithmetic of
 * csrc/bc6h_decode_core.h on the host, for callers without a GPU and for the tests.  Nothing is done for a NULL pointer or an extent of 0. */
void PBR_DecodeBC6HBlocks(const void* blocks, uint32_t w, uint32_t h, uint16_t* rgb_half);

typedef struct PBR_GeometryPass PBR_GeometryPass;
/* the two render passes and pipelines of the reference: pass i writes gb's four colour planes, PBR_PostVelocity(pp, i) and gb->depth */
PBR_GeometryPass* PBR_MakeGeometryPass(const PBR_GBuffer* gb, PBR_PostProcess* pp, uint32_t width, uint32_t height);
void PBR_DestroyGeometryPass(PBR_GeometryPass* pass);
GPU_Buffer* PBR_GeometryGlobalsBuffer(PBR_GeometryPass* pass);              /* persistently mapped PBR_Globals */
GPU_GraphicsPipeline* PBR_GeometryPipeline(PBR_GeometryPass* pass, uint32_t frame_idx_mod2);
GPU_RenderPass* PBR_GeometryRenderPass(PBR_GeometryPass* pass, uint32_t frame_idx_mod2);
GPU_PipelineLayout* PBR_GeometryLayout(PBR_GeometryPass* pass);             /* GLOBALS, TEX0, TEX1, TEX_ORM, TEX_EMISSIVE, SAMPLER_LINEAR_WRAP */
/* the set a part with this material draws with; created on first use and kept until the pass is destroyed, so destroy the pass
 * before any material it has seen */
GPU_DescriptorSet* PBR_GeometryDescriptorSet(PBR_GeometryPass* pass, PBR_Material* material);
/* render.cpp:991, :993, :1076-1115: copies globals (if not NULL), clears the depth, draws every part of `mesh` and then of `skybox`
 * (may be NULL) with its own buffers.  A part that has no material (PBR_MeshSetPartMaterial) is not drawn.  jitter / jitter_prev: two
 * floats each (NULL = 0, 0).  Materials must outlive the pass: it keeps one descriptor set per material it has drawn with. */
void PBR_RecordGeometryPass(PBR_GeometryPass* pass, GPU_Graph* graph, const PBR_Mesh* mesh, const PBR_Mesh* skybox, const PBR_Globals* globals,
                            const float* jitter, const float* jitter_prev, uint32_t frame_idx);

/* ---- voxelise pass (N7 / K14): render.cpp:113-149 (pipeline: lightgrid_voxelize.glsl, conservative rasterisation), :711-714 (an
 *      N x N render pass without targets), asset_import.cpp:196-204 (a part's descriptor set), render.cpp:1039-1056 (one GPU_OpDraw per
 *      part).  It stores lit surface colour into the grid of `lightgrid` and reads the depth map of `sun`; both must outlive the pass.
 *      The frame-0 clear stays PBR_RecordLightgridClear. ---- */
typedef struct PBR_VoxelizePass PBR_VoxelizePass;
PBR_VoxelizePass* PBR_MakeVoxelizePass(PBR_Lightgrid* lightgrid, PBR_SunDepthPass* sun);
void PBR_DestroyVoxelizePass(PBR_VoxelizePass* pass);
GPU_Buffer* PBR_VoxelizeGlobalsBuffer(PBR_VoxelizePass* pass);              /* persistently mapped PBR_Globals */
GPU_GraphicsPipeline* PBR_VoxelizePipeline(PBR_VoxelizePass* pass);
GPU_RenderPass* PBR_VoxelizeRenderPass(PBR_VoxelizePass* pass);
/* GLOBALS, SSBO0, SSBO1, IMG0, SUN_DEPTH_MAP, TEX0, TEX_EMISSIVE, SAMPLER_PERCENTAGE_CLOSER, SAMPLER_LINEAR_WRAP: bindings 0 .. 8 */
GPU_PipelineLayout* PBR_VoxelizeLayout(PBR_VoxelizePass* pass);
GPU_Sampler* PBR_VoxelizeShadowSampler(PBR_VoxelizePass* pass);             /* linear, clamp, GPU_CompareOp_Less (render.cpp:664-673) */
/* the set a part of `mesh` with this material draws with; created on first use and kept until the pass is destroyed, so destroy the
 * pass before any mesh or material it has seen */
GPU_DescriptorSet* PBR_VoxelizeDescriptorSet(PBR_VoxelizePass* pass, const PBR_Mesh* mesh, PBR_Material* material);
/* render.cpp:991, :1039-1056: copies globals (if not NULL) and draws every part of `mesh` that has a material */
void PBR_RecordVoxelizePass(PBR_VoxelizePass* pass, GPU_Graph* graph, const PBR_Mesh* mesh, const PBR_Globals* globals);

#ifdef __cplusplus
}
#endif
#endif
