/*
 * gpux.h -- extensions of the HIP backend beyond the reference's GPU_* API (new names only; nothing
 * in gpu_hip.h changes meaning).  They exist for what the reference cannot express:
 * multi-GPU sharding (dispatch of a (face,row) sub-range, device selection), reading back mips
 * other than 0 (the reference's GPU_OpCopyTextureToBuffer is mip-0 only, gpu_vulkan.c:2945-2951),
 * parameterised sizes/sample counts (literals inside the reference shaders), per-op HIP-event
 * timing, and handing device pointers to a communication library (RCCL).
 */
#ifndef GPUX_H
#define GPUX_H

#include "gpu_hip.h"

/* ---- device / errors ---- */
GPU_API void GPUX_SetDevice(int hip_device_index);        /* call before GPU_Init; default: $LOCAL_RANK or 0 */
GPU_API int  GPUX_GetDevice(void);
typedef void (*GPUX_ErrorHandler)(const char* message, void* user);
/* With a handler installed, a failing GPU_* call reports and returns (NULL / no-op) instead of aborting. */
GPU_API void GPUX_SetErrorHandler(GPUX_ErrorHandler handler, void* user);
GPU_API const char* GPUX_BackendName(void);               /* "hip-gfx950" */

/* ---- push-constant block understood by the IBL kernels when size == sizeof(GPUX_IBLConstants).
 * A 4-byte block keeps the reference meaning (int mip_level; gen_prefiltered_env_map.glsl:99-101):
 * roughness = {0,.03,.15,.4,.6}[mip] (mips >= 5: min(1, .6 + .08*(mip-4)), an extension),
 * source LOD = 1 for mip 0 else 3 + mip (clamped to the env chain), 8192 samples. ---- */
typedef struct GPUX_IBLConstants {
    int32_t mip_level;        /* prefilter: which branch (0 = copy, else Monte-Carlo) */
    float   roughness;        /* prefilter MC roughness */
    float   src_lod;          /* integer-valued source LOD */
    int32_t sample_count;     /* 0 = shader default (8192 prefilter / 1024 irradiance / 4096 LUT) */
} GPUX_IBLConstants;

/* ---- sub-range dispatch: like GPU_OpDispatch over the bound OUTPUT image, restricted to faces
 * [face0,face1) and rows [row0,row1) (rows of the LUT for gen_brdf_integration_map). ---- */
GPU_API void GPUX_OpDispatchRows(GPU_Graph* graph, uint32_t face0, uint32_t face1, uint32_t row0, uint32_t row1);
/* the same for the light-grid sweep pipeline (lightgrid_sweep.glsl): invocations (iy, iz) in [y0,y1) x [z0,z1),
 * where GPU_OpDispatch(1, gy, gz) covers [0, 8 gy) x [0, 8 gz); the direction comes from the push constant. */
GPU_API void GPUX_OpDispatchLines(GPU_Graph* graph, uint32_t y0, uint32_t y1, uint32_t z0, uint32_t z1);

/* ---- shade pass controls ---- */
enum { GPUX_Shade_IBL = 1 << 0, GPUX_Shade_LightShafts = 1 << 1,
       GPUX_Shade_SunShadows = 1 << 2, /* SUN_DEPTH_MAP: 4-tap PCF sun shadow + shaft visibility (lighting_pass.glsl:594-608, 646) */
       GPUX_Shade_VoxelGI = 1 << 3,    /* LIGHTGRID + PREV_FRAME_RESULT + GBUFFER_DEPTH: the live ambient / specular traces (:273-424, :685, :701);
                                          with LightShafts | SunShadows | VoxelGI the pass is the reference's complete live shader */
       GPUX_Shade_SH9Irradiance = 1 << 4 /* with GPUX_Shade_IBL: the ambient term from the 27 SH9 coefficients of GPUX_SetShadeSH9 in place of
                                          TEX_IRRADIANCE_MAP, which may stay unbound (csrc/sh_shade_core.h, DESIGN.md 4 "K5, SH9 ambient") */ };
GPU_API void GPUX_SetShadeFlags(GPU_GraphicsPipeline* pipeline, int flags);    /* default GPUX_Shade_IBL */
GPU_API int GPUX_GetShadeFlags(GPU_GraphicsPipeline* pipeline);
/* The coefficients GPUX_Shade_SH9Irradiance shades from: 27 doubles (216 bytes, index 3 k + c: what GPUX_OpProjectSH9 writes) at `offset`
 * (a multiple of 8) of `coef`; NULL unsets them.  A draw recorded with the flag keeps the buffer and offset it was recorded with; the
 * numbers are read on the device when the draw executes, after every earlier op of its graph and of the graphs submitted before it.
 * A device buffer (GPU_BufferFlag_GPU) keeps them in the cache: every workgroup of the draw reads them. */
GPU_API void GPUX_SetShadeSH9(GPU_GraphicsPipeline* pipeline, GPU_Buffer* coef, uint32_t offset);
/* full-screen draw restricted to rows [row0,row1) (screen-band sharding) */
GPU_API void GPUX_OpDrawRows(GPU_Graph* graph, uint32_t row0, uint32_t row1);

/* ---- transfers the reference API lacks ---- */
GPU_API void GPUX_OpCopyTextureMipToBuffer(GPU_Graph* graph, GPU_Texture* src, uint32_t mip_level, GPU_Buffer* dst, uint32_t dst_offset);
GPU_API void GPUX_OpCopyBufferToTextureMip(GPU_Graph* graph, GPU_Buffer* src, uint32_t src_offset, GPU_Texture* dst, uint32_t mip_level);
GPU_API uint64_t GPUX_TextureMipBytes(const GPU_Texture* texture, uint32_t mip_level);   /* all layers of one mip */
/* K15: a 2-D BC1 / BC3 / BC5 texture keeps its blocks (the copies above move those, format-true) and owns a decoded RGBA8UN image
 * that the draws sample; a level is decoded when GPU_MakeTexture(data), GPU_OpCopyBufferToTexture or GPUX_OpCopyBufferToTextureMip
 * writes it (memory written behind the backend's back is not followed).  This copies one level of the decoded image
 * (width x height x 4 bytes, tight rows) into a buffer, for tests; any other texture is an error. */
GPU_API void GPUX_OpCopyDecodedTextureMipToBuffer(GPU_Graph* graph, GPU_Texture* src, uint32_t mip_level, GPU_Buffer* dst, uint32_t dst_offset);
/* K17: the SH9 form of an environment's diffuse lighting (csrc/sh_core.h), as graph ops so that they order with
 * everything else recorded on the graph.  Source and target are square RGBA32F cubemaps.
 * Project: faces [face0, face1) x rows [row0, row1) of one level -> 27 doubles (216 bytes, index 3 k + c; offset a multiple of 8):
 * the partial sum of those rows -- callers add partials themselves.  Deterministic: the same op gives the same bytes.
 * IrradianceFromSH9: the whole level from 27 doubles, E / (2 pi) like K3, alpha 0, NOT clamped (the series may ring negative).
 * Both are plain launches and may be captured under GPUX_SetGraphReplay(1). */
GPU_API void GPUX_OpProjectSH9(GPU_Graph* graph, GPU_Texture* cube, uint32_t mip_level, uint32_t face0, uint32_t face1, uint32_t row0, uint32_t row1,
                               GPU_Buffer* dst, uint32_t dst_offset);
GPU_API void GPUX_OpIrradianceFromSH9(GPU_Graph* graph, GPU_Buffer* src, uint32_t src_offset, GPU_Texture* irradiance_cube, uint32_t mip_level);
/* K18: one level (every layer) of a 2-D or cube RGBA32F / RGBA16F texture -> BC6H_UF16 blocks (mode 11; csrc/bc6h_core.h)
 * at dst_offset (a multiple of 16): ceil(w / 4) x ceil(h / 4) blocks of 16 bytes per layer, row-major, layer after layer --
 * GPUX_BC6HMipBytes in all (0 for a texture the op does not take).  A plain launch, ordered with the rest of the graph; may be captured
 * under GPUX_SetGraphReplay(1). */
GPU_API void GPUX_OpEncodeBC6H(GPU_Graph* graph, GPU_Texture* src, uint32_t mip_level, GPU_Buffer* dst, uint32_t dst_offset);
GPU_API uint64_t GPUX_BC6HMipBytes(const GPU_Texture* texture, uint32_t mip_level);
/* K18 with a quality level.  GPUX_BC6H_OneRegion records exactly what GPUX_OpEncodeBC6H records.  GPUX_BC6H_TwoRegions is an op of its
 * own (K18.bc6h_encode2 in the per-op times): per block the one-region block or, where it has a strictly lower squared error, one of
 * the two-region cases 0, 14, 1, 30 over the best of the 32 partitions (csrc/bc6h2_core.h, DESIGN.md "K18, two regions"); same
 * layout, same size, several times the time.  Any other quality is one more error at record time with nothing recorded. */
enum { GPUX_BC6H_OneRegion = 0, GPUX_BC6H_TwoRegions = 1 };
GPU_API void GPUX_OpEncodeBC6HEx(GPU_Graph* graph, GPU_Texture* src, uint32_t mip_level, GPU_Buffer* dst, uint32_t dst_offset, uint32_t quality);
/* K19: the way back: GPUX_BC6HMipBytes(dst, mip_level) bytes of BC6H_UF16 blocks (any of the 14 modes; csrc/bc6h_decode_core.h, DESIGN.md
 * K19) at src_offset (a multiple of 16), laid out as GPUX_OpEncodeBC6H writes them -> one level, every layer, of a 2-D or cube RGBA32F /
 * RGBA16F texture; alpha 1.  A texture writer like any other: the target's sampler twins are rebuilt before the next use.  Anything
 * else is one error at record time with nothing recorded.  A plain launch; may be captured under GPUX_SetGraphReplay(1). */
GPU_API void GPUX_OpDecodeBC6H(GPU_Graph* graph, GPU_Buffer* src, uint32_t src_offset, GPU_Texture* dst, uint32_t mip_level);
/* K20: level src_mip of an RGBA32F cubemap (any face size) -> level dst_mip of a 2-D RGBA32F or RGBA16F texture as a lat-long panorama;
 * that level's extent (1 .. 16384 a side, nothing has to be a multiple of anything) is the panorama's.  Pixel (x, y) is the seamless
 * bilinear sample of the cube level along d = (sin t cos p, sin t sin p, cos t), p = ((2 x + 1) / w - 1) pi, t = (2 y + 1) / (2 h) pi:
 * Z-up, row 0 next to +Z, the inverse of K6 (csrc/panorama_core.h).  No minification filter: a panorama far narrower
 * than 4 n aliases, and the choice of level is the caller's.  The column / row tables are built and uploaded when the op is recorded
 * and belong to the graph; the apron of the cube is ensured from src_mip when the op executes (its own timed entry, apron.panorama,
 * in front of K20.cube_to_panorama).  Reads the cube and writes dst, both followed: a later sampler of dst sees the new bytes, a later
 * write to the cube has the next submission rebuild the apron.  Never captured: a graph holding this op submits the plain way under
 * GPUX_SetGraphReplay(1).  Any bad argument (NULL, formats, a cube or 3-D target, a mip out of range, inside a render pass, an extent
 * above 16384) is one error at record time with nothing recorded. */
GPU_API void GPUX_OpCubeToPanorama(GPU_Graph* graph, GPU_Texture* cube, uint32_t src_mip, GPU_Texture* dst, uint32_t dst_mip);
/* The width * height * 3 fp32 directions K20 samples along, row-major: the arithmetic of the op's tables (the same translation unit),
 * pure host code, callable without GPU_Init.  For tools that must find the pixel of a direction, and for tests.  0 on success, 1 for a
 * NULL pointer or an extent outside 1 .. 16384. */
GPU_API int GPUX_PanoramaDirections(uint32_t width, uint32_t height, float* xyz);
/* K21: faces [face0, face1) x rows [row0, row1) of level dst_mip of an RGBA32F cubemap from ANOTHER RGBA32F cubemap and its mip chain
 * by GGX importance sampling with filtered lookups (csrc/prefilter_ggx_core.h): sample_count (1 .. 4096) GGX-distributed
 * light directions for V = N = the texel's direction at `roughness` (0 < r <= 1), each a trilinear seamless sample of env_cube at the
 * level whose texel solid angle matches the sample's, plus lod_bias (finite; 1 is the usual choice), weighted by N.L and divided by
 * the weight sum; alpha 1.  Any face size, any number of source levels.  The sample table is built and uploaded when the op is
 * recorded and belongs to the graph; the whole apron of env_cube is ensured when the op executes (its own timed entry,
 * apron.prefilter_ggx, in front of K21.prefilter_ggx.mip<dst_mip>).  Reads env_cube and writes dst_cube, both followed.  A texel's
 * bytes depend on neither the range it was dispatched in nor the run; texels outside the range are not touched.  Never captured:
 * a graph holding this op submits the plain way under GPUX_SetGraphReplay(1).  Not part of the level-overlap regions of K3 / K4.
 * With an odd sample_count at roughness 1 the middle sample has weight 0 and is dropped; sample_count 1 then keeps none and the
 * level is 0 / 0.  Any bad argument (NULL, formats, not a cube, the same texture twice, a mip out of range, roughness outside (0, 1]
 * or NaN, a count outside 1 .. 4096, a bias that is not finite, an empty or out-of-range face / row range, inside a render pass) is
 * one error at record time with nothing recorded. */
GPU_API void GPUX_OpPrefilterGGX(GPU_Graph* graph, GPU_Texture* env_cube, GPU_Texture* dst_cube, uint32_t dst_mip,
                                 float roughness, uint32_t sample_count, float lod_bias,
                                 uint32_t face0, uint32_t face1, uint32_t row0, uint32_t row1);
/* The sample table K21 uses for a source of src_levels levels (1 .. the full chain) below a src_size^2 level 0: *kept entries
 * {l.x, l.y, l.z, lod} in xyz_lod (room for 4 * sample_count floats) and the weight sum.  The arithmetic of the op's table (the same
 * translation unit), pure host code, callable without GPU_Init.  0 on success, 1 for a NULL pointer or an argument the op refuses. */
GPU_API int  GPUX_PrefilterGGXSamples(float roughness, uint32_t sample_count, uint32_t src_size, uint32_t src_levels,
                                      float lod_bias, float* xyz_lod /* 4 * sample_count */, uint32_t* kept, float* wsum);
/* K22: rows [row0, row1) of level 0 of a 2-D RG16F / RG32F / RGBA32F texture as the split-sum BRDF LUT of the GGX lobe by importance
 * sampling (Karis' IntegrateBRDF; csrc/brdf_lut_ggx_core.h), the LUT that goes with K21's specular cube: texel (x, y)
 * holds (A, B) -- specular = prefiltered * (F0 * A + B) -- at N.V = (x + .5) / width and roughness (y + .5) / height, from sample_count
 * (1 .. 4096) GGX-distributed half vectors; RGBA32F stores (A, B, 0, 1).  Any extent from 1 to 4096 on each axis, square or not.
 * `visibility` selects the geometry term.  The sample table is built and uploaded when the op is recorded and belongs to the graph;
 * nothing is allocated when the op executes, so the op may be captured under GPUX_SetGraphReplay(1).  Writes lut_tex, followed: the
 * sampler twin the lighting pass built from the old bytes is dropped.  Timed as K22.brdf_lut_ggx.  A texel's bytes depend on neither
 * the rows it was dispatched with nor the run; texels outside the rows are not touched.  Any bad argument (NULL, another format, a cube,
 * layered or 3-D texture, an extent above 4096, a count outside 1 .. 4096, an unknown visibility, an empty or out-of-range row range,
 * inside a render pass) is one error at record time with nothing recorded. */
typedef enum GPUX_BrdfLutVisibility {
    GPUX_BrdfLut_SmithSchlick = 0,      /* G1(N.V) G1(N.L), G1(c) = c / (c (1 - k) + k), k = roughness^2 / 2: lighting_pass.glsl's GeometrySmithIBL */
    GPUX_BrdfLut_SmithCorrelated = 1    /* the height-correlated Smith term (Heitz), as in Filament's DFG */
} GPUX_BrdfLutVisibility;
GPU_API void GPUX_OpBrdfLutGGX(GPU_Graph* graph, GPU_Texture* lut_tex, uint32_t sample_count, uint32_t visibility, uint32_t row0, uint32_t row1);
/* The sample table K22 uses: {xi1, cos phi, sin phi} per sample into xi_cos_sin (room for 3 * sample_count floats).  The arithmetic of
 * the op's table (the same translation unit), pure host code, callable without GPU_Init.  0 on success, 1 for a NULL pointer or a count
 * outside 1 .. 4096. */
GPU_API int  GPUX_BrdfLutGGXSamples(uint32_t sample_count, float* xi_cos_sin /* 3 * sample_count */);
GPU_API void* GPUX_TextureDevicePtr(GPU_Texture* texture, uint32_t mip_level);            /* for RCCL / interop */
GPU_API void* GPUX_BufferDevicePtr(GPU_Buffer* buffer);
GPU_API void* GPUX_GraphStream(GPU_Graph* graph);                                         /* hipStream_t */

/* ---- textures over caller-owned HBM (e.g. a torch tensor that RCCL gathers into): same layout as GPU_MakeTexture,
 * [mip][layer][y][x] tight; the caller keeps the allocation alive and frees it after GPU_DestroyTexture. ---- */
GPU_API GPU_Texture* GPUX_MakeTextureExternal(GPU_Format format, uint32_t width, uint32_t height, uint32_t depth, GPU_TextureFlags flags,
                                              void* device_memory, uint64_t device_bytes);
/* Tell the backend that the texture's memory was written behind its back (RCCL receive, torch, any other library working on
 * GPUX_TextureDevicePtr / external memory): everything built lazily from the texture (apron, cells of every level, LUT cells, the
 * per-level range of GPUX_SetPrefilterTolerance) is dropped, exactly as after an op that writes it, and rebuilt before the next use. */
GPU_API void GPUX_InvalidateTexture(GPU_Texture* texture);
GPU_API uint64_t GPUX_TextureTotalBytes(const GPU_Texture* texture);
GPU_API uint64_t GPUX_TextureMipOffset(const GPU_Texture* texture, uint32_t mip_level);

/* ---- equirectangular input (extension; the reference only loads cube strips): uploads the RGBA32F panorama, converts it
 * to a face_size^2 cubemap (K6) and generates the mip chain before returning, like GPU_MakeTexture(data != NULL). ---- */
GPU_API GPU_Texture* GPUX_MakeCubemapFromEquirect(const void* rgba32f, uint32_t width, uint32_t height, uint32_t face_size, GPU_TextureFlags extra_flags);

/* ---- per-op timing with HIP events on the graph's own stream ---- */
GPU_API void GPUX_EnableOpTiming(int enable);
GPU_API uint32_t GPUX_GraphTimedOpCount(GPU_Graph* graph);          /* ops of the last waited submission */
GPU_API const char* GPUX_GraphTimedOpName(GPU_Graph* graph, uint32_t index);
GPU_API float GPUX_GraphTimedOpMs(GPU_Graph* graph, uint32_t index);
/* ---- tolerance-budgeted sample cut of the specular prefilter (opt-in, NEVER the default: the reference sums every sample) ----
 * The Monte-Carlo weights of a low-roughness level decay like exp(-i / 14.7): of mip 1's 1389 non-zero fp32 weights the last ~900
 * together carry less than 1e-13 of the sum.  With rel > 0 a prefilter dispatch keeps the first K samples, K the smallest count with
 *     (sum of dropped weights) * max(source level)  <=  rel * (sum of kept weights) * min(source level)
 * -- a rigorous bound on every texel's relative error (taps are convex combinations of the level's texels), evaluated on the host
 * from the weight table and the level's measured range (one reduction + read-back per source level and content change).  A level
 * with a zero or negative texel is never cut.  rel = 0 (default) restores the exact sum.  GPUX_PrefilterKeptSamples(mip): what the
 * last dispatch of that output mip kept (0: none recorded). */
GPU_API void GPUX_SetPrefilterTolerance(float rel);
GPU_API int GPUX_PrefilterKeptSamples(uint32_t mip_level);
/* busy span of the last waited submission on the graph's main stream: one event pair from before its first op to after the
 * last join of its side streams (overlapping dispatches are not counted twice, unlike the sum of the per-op times) */
GPU_API float GPUX_GraphSpanMs(GPU_Graph* graph);

/* ---- overlap of small precompute dispatches: consecutive row-ranged K3/K4 dispatches (GPUX_OpDispatchRows) of fewer than
 * 2M texels whose outputs are disjoint and that do not read each other's output are spread over `count` side streams
 * between a fork and a join event; anything else executes in recording order on the graph's stream.  0 or 1 turns it off,
 * a negative count restores the default (environment PBR_TILE_STREAMS, else 4).  Results do not depend on the setting. ---- */
GPU_API void GPUX_SetTileStreams(int count);
/* ---- whole levels side by side: a run of at least two consecutive K3/K4 dispatches of whole levels (GPUX_OpDispatchRows over every
 * row, or GPU_OpDispatch) that pass the same independence check runs as one region, largest dispatch first, each on the least loaded
 * of `count` streams, the graph's own among them (2 .. the GPUX_SetTileStreams value; below 2: the default, 2).  on = 0: whole levels stay a serial chain.
 * GPUX_SetTileStreams(0 or 1) turns this off too.  GPUX_LevelOverlapCount: dispatches the last submission placed this way.  Inside
 * a region a timed op's figure is its span beside its neighbours; GPUX_GraphSpanMs is the job's.  Results do not depend on any of it. ---- */
GPU_API void GPUX_SetLevelOverlap(int on);
GPU_API void GPUX_SetLevelStreams(int count);
GPU_API uint32_t GPUX_LevelOverlapCount(void);

/* ---- hipGraph replay of the per-frame chain: with replay on, GPU_GraphSubmit captures the launches of a graph whose ops are all
 * launch-only (light-grid sweep, draws of the shade / TAA / bloom / tone-map pipelines, blits, memset clears, mip generation) and
 * whose sampler twins already exist into a hipGraph, updates the executable graph kept from this GPU_Graph's previous submission
 * in place (same chain, new arguments) and launches it: one dispatch of ~25 dependent kernels instead of 25.  Every other graph, and
 * every submission while per-op timing is on, runs as before.  Results are identical.  enable < 0: environment PBR_GRAPH_REPLAY, else off. ---- */
GPU_API void GPUX_SetGraphReplay(int enable);
GPU_API void GPUX_GraphReplayStats(GPU_Graph* graph, uint64_t* launches, uint64_t* updates, uint64_t* instantiations);
/* 1:1 blits folded into the additive bloom draw that consumes their copy, since the library was loaded (env PBR_GRAPH_FOLD=0 keeps every blit) */
GPU_API uint64_t GPUX_FoldedBlitCount(void);
/* Graphs in flight: the leading ops of a graph that share no texture with the TAIL of the graph submitted before it (from its first bloom
 * draw on) start once that graph's head is done instead of after its end (GPU_GraphSubmit); everything else keeps submission order.
 * on: 1 / 0, -1 = default (env PBR_GRAPH_OVERLAP, else 1).  GPUX_OverlappedSubmitCount: submissions that started this way. */
GPU_API void GPUX_SetGraphOverlap(int on);
GPU_API uint64_t GPUX_OverlappedSubmitCount(void);

/* ---- K12: the sun depth pass (sun_depth_pass.glsl through GPU_OpDrawIndexed).  Triangles the rasteriser skipped since
 * the library was loaded: a vertex index past the bound vertex buffer, a non-finite transformed vertex, or a vertex outside the
 * +-2^21-pixel guard band (where Vulkan would clip).  Counted on the device; the value includes every submission waited for. ---- */
GPU_API uint64_t GPUX_RasterRejectedTriangles(void);
/* fragments the voxelise pass (K14) kept since GPU_Init: the stores lightgrid_voxelize.glsl would have issued (synchronises) */
GPU_API uint64_t GPUX_VoxelizeFragments(void);

#endif
