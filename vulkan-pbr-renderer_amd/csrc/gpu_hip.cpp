// gpu_hip.cpp -- HIP / gfx950 implementation of the GPU_* boundary declared in include/gpu_hip.h.
//
// Takes the place of src/gpu/gpu_vulkan.c for the IBL-precompute and shade hot path:
//   * textures/buffers are linear HBM allocations (cube = [mip][face][y][x], tight);
//   * sampled cubes carry a lazily rebuilt "bordered" twin (seamless-filter apron, k_cube.hip);
//   * descriptor sets are plain slot arrays resolved by binding NAME at launch;
//   * compute / graphics pipelines resolve to built-in kernels by shader identity;
//   * a graph is a HIP stream plus a recorded op list, launched at GPU_GraphSubmit.
// Error convention follows gpu_vulkan.c:6-8,387-392: print "GPU-ERROR: ..." and trap, unless a
// handler was installed through GPUX_SetErrorHandler.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "gpux.h"
#include "pbr_kernels.h"
#include "panorama_core.h"
#include "prefilter_ggx_core.h"
#include "brdf_lut_ggx_core.h"

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
static GPUX_ErrorHandler g_err_handler = nullptr;
static void* g_err_user = nullptr;

static void gpu_fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (g_err_handler) { g_err_handler(buf, g_err_user); return; }
    fprintf(stderr, "GPU-ERROR: %s\n", buf);
    fflush(stderr);
    abort();
}
#define GPU_REQUIRE(cond, ret, ...) do { if (!(cond)) { gpu_fail(__VA_ARGS__); return ret; } } while (0)
#define GPU_REQUIRE_V(cond, ...) do { if (!(cond)) { gpu_fail(__VA_ARGS__); return; } } while (0)
#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { gpu_fail("%s: HIP call failed: %s (%s)", __func__, #call, hipGetErrorString(e_)); } } while (0)

// ------------------------------------------------------------------------------------------
// object model
// ------------------------------------------------------------------------------------------
enum BindKind { Bind_Texture, Bind_Sampler, Bind_Buffer, Bind_StorageImage };
enum KernelId { Kernel_None = 0, Kernel_BrdfLut, Kernel_Irradiance, Kernel_Prefilter, Kernel_Lighting, Kernel_LightgridSweep, Kernel_TaaResolve, Kernel_FinalPost, Kernel_BloomDown, Kernel_BloomUp, Kernel_SunDepth, Kernel_Geometry, Kernel_Voxelize };

// the full-screen passes behind the lighting pass (K8 .. K11), and the two of them that make the bloom chain
static bool is_bloom_kernel(KernelId k) { return k == Kernel_BloomDown || k == Kernel_BloomUp; }
static bool is_post_kernel(KernelId k) { return is_bloom_kernel(k) || k == Kernel_FinalPost || k == Kernel_TaaResolve; }

struct GPU_Sampler { GPU_SamplerDesc desc; bool shared; };

struct LayoutBinding { std::string name; BindKind kind; GPU_Format format; };
struct GPU_PipelineLayout { std::vector<LayoutBinding> bindings; bool finalized = false; };

struct TextureImpl {
    GPU_Texture base;                 // public part first (gpu_vulkan.c:182-205 does the same)
    void* dev = nullptr;              // [mip][layer][z][y][x]
    size_t bytes = 0;
    std::vector<size_t> mip_offset;   // bytes
    uint32_t texel_bytes = 0;
    bool owns_memory = true;          // false: GPUX_MakeTextureExternal (caller-owned HBM, e.g. a torch tensor)
    // BC1 / BC3 / BC5 2-D textures (K15): `dev` keeps the compressed blocks; `decoded` is what the draws sample -- RGBA8UN, all levels
    // back to back like an RGBA8UN texture of the same extents.  Not lazily invalidated: exec_copy decodes a level when it is written
    void* decoded = nullptr; std::vector<size_t> decoded_offset;
    // What the hot kernels sample in place of `dev`: built on demand (ensure_*, level_range), each part by its own flag alone;
    // marked stale by texture_written() only -- all of it, after every op that writes the texture (exec_op); freed by free_derived()
    struct Derived {
        // bordered pyramid twin (RGBA32F cubes only), the seamless-filter apron: valid for levels >= bordered_from
        void* bordered = nullptr; bool bordered_valid{}; int bordered_from = 0;
        // 2x2-footprint "cells" twin of the levels with n <= 512 (levels cells_first.., back to back), built per level from the apron
        void* cells = nullptr; int cells_first = 0; std::vector<size_t> cells_off; std::vector<char> cells_valid;
        void* lut_cells = nullptr; bool lut_cells_valid{};          // RG16F 2-D textures sampled by the shade pass
        std::vector<char> range_valid; std::vector<float> range_min, range_max; void* range_dev = nullptr;   // {min, max} of a level's RGB values (level_range)
    } derived;
};
static void texture_written(TextureImpl* t) {
    TextureImpl::Derived& d = t->derived;
    d.bordered_valid = false; d.lut_cells_valid = false;
    std::fill(d.cells_valid.begin(), d.cells_valid.end(), 0); std::fill(d.range_valid.begin(), d.range_valid.end(), 0);
}
static void free_derived(TextureImpl* t) {
    for (void* p : {t->derived.bordered, t->derived.cells, t->derived.lut_cells, t->derived.range_dev}) (void)hipFree(p);   // NULL: a no-op
    t->derived = TextureImpl::Derived();
}
struct BufferImpl {
    GPU_Buffer base;
    void* dev = nullptr;              // device-visible pointer (== base.data for CPU buffers)
    bool pinned_host = false;
};

struct Slot { BindKind kind; bool set = false; TextureImpl* tex = nullptr; uint32_t mip = 0; bool whole = true;
              GPU_Sampler* sampler = nullptr; BufferImpl* buf = nullptr; };
struct GPU_DescriptorSet { GPU_PipelineLayout* layout; std::vector<Slot> slots; bool finalized = false; GPU_DescriptorArena* arena = nullptr; };
struct GPU_DescriptorArena { std::vector<GPU_DescriptorSet*> sets; };

struct GPU_ComputePipeline { GPU_PipelineLayout* layout; KernelId kernel; };
struct GPU_RenderPass { GPU_RenderPassDesc desc; std::vector<GPU_TextureView> targets; };
struct GPU_GraphicsPipeline { GPU_PipelineLayout* layout; GPU_RenderPass* pass; KernelId kernel; int shade_flags; bool blend_additive = false;
                              uint32_t vertex_stride = 0; /* raster kinds: bytes per vertex (gpu_vulkan.c:1745-1762) */
                              const struct RasterKind* raster = nullptr; /* K12 / K13 / K14: the row of its raster kind */
                              BufferImpl* sh9_buf = nullptr; uint32_t sh9_offset = 0; /* GPUX_SetShadeSH9 */ };

enum OpKind { Op_Dispatch, Op_Shade, Op_MipGen, Op_CopyB2T, Op_CopyT2B, Op_CopyB2B, Op_Blit, Op_Clear, Op_Raster, Op_CopyDecodedT2B, Op_ProjectSH9, Op_IrradianceSH9, Op_EncodeBC6H, Op_DecodeBC6H, Op_CubeToPanorama, Op_PrefilterGGX, Op_BrdfLutGGX };
// one draw of a raster job: job triangles from first_tri on, matrices from the set's GLOBALS, the buffers and the target its kind
// names (K12 / K13: the buffers bound at the draw; K14: SSBO0 / SSBO1 of the set, first_index = its first vertex) and the pushed
// constants (K13 reads them: the skybox rebinds both inside the pass)
struct RasterDraw { GPU_DescriptorSet* set; uint32_t first_tri, first_index, vertex_offset; BufferImpl* vb = nullptr; BufferImpl* ib = nullptr; TextureImpl* target = nullptr; float push[4] = {0, 0, 0, 0}; };
struct Op {
    OpKind kind;
    std::string name;
    // dispatch
    GPU_ComputePipeline* cpipe = nullptr;
    GPU_DescriptorSet* set = nullptr;
    uint8_t push[128]; uint32_t push_size = 0;
    uint32_t face0 = 0, face1 = 6, row0 = 0, row1 = 0;
    bool rows_explicit = false;
    uint32_t gx = 0, gy = 0, gz = 0;
    // shade (a lighting draw recorded under GPUX_Shade_SH9Irradiance: buf / off_a = its 27 coefficients, else buf == nullptr)
    GPU_GraphicsPipeline* gpipe = nullptr;
    GPU_RenderPass* pass = nullptr;
    // transfers
    TextureImpl* tex = nullptr; TextureImpl* tex2 = nullptr;
    BufferImpl* buf = nullptr; BufferImpl* buf2 = nullptr;
    uint32_t mip = 0, mip2 = 0, layer0 = 0, layer_count = 0, layer2 = 0;
    uint64_t off_a = 0, off_b = 0, size = 0;
    float clear[4]; uint32_t cleari[4]; int clear_mode = 0;
    uint32_t quality = 0;                          // Op_EncodeBC6H: GPUX_BC6H_OneRegion / GPUX_BC6H_TwoRegions
    const void* pano_table = nullptr;              // Op_CubeToPanorama: the op's column / row table (GPU_Graph::pano)
    const void* ggx_table = nullptr; uint32_t ggx_kept = 0; float ggx_wsum = 0.0f;   // Op_PrefilterGGX: its sample table (GPU_Graph::pano too)
    const void* lut_table = nullptr; uint32_t lut_samples = 0, lut_visibility = 0;   // Op_BrdfLutGGX: its sample table (the same), count and term
    // submit-time folding (fold_blits): a 1:1 blit whose copy is consumed only by an additive bloom draw onto its target is not
    // executed; that draw takes the blend operand from the blit's source instead
    bool folded = false;
    TextureImpl* blend_tex = nullptr; uint32_t blend_mip = 0;
    bool skip_level0 = false;                      // Op_Clear of all levels whose level 0 the next op overwrites entirely
    // raster job (Op_Raster, kind: gpipe->raster): the draws of one render-pass instance that go together; tex = depth target (K14: the
    // light grid), buf = vertices and buf2 = indices of the job's first draw (K12 has one pair per job)
    std::vector<RasterDraw> draws;
    uint32_t tri_count = 0;
    int raster_slot = -1;                          // GPU_Graph::raster scratch of this job
};
struct DrawParams { GPU_GraphicsPipeline* pipeline; GPU_DescriptorSet* set; };
// per raster job of a graph, kept across submissions: bins / records (device), the draw table (device + pinned staging)
struct RasterScratch { void* dev = nullptr; size_t dev_bytes = 0; void* draws_dev = nullptr; void* draws_host = nullptr; size_t draws_cap = 0; /* bytes */ };

struct GPU_Graph {
    hipStream_t stream = nullptr;
    hipStream_t cur = nullptr;                     // stream the op being executed launches on (stream, or a side stream)
    std::vector<hipStream_t> side;                 // side streams for overlapping independent tile dispatches (created on first use)
    std::vector<hipEvent_t> sync_ev;               // untimed fork/join events
    hipEvent_t order_ev = nullptr;                 // recorded on this graph's stream when the NEXT submitted graph must follow it
    // head / tail split of the last submission (GPU_GraphSubmit): `mid_ev` is recorded in front of the first bloom draw; the next graph's
    // leading ops that touch none of the textures in tail_reads / tail_writes wait for it instead of for the whole graph
    hipEvent_t mid_ev = nullptr;
    bool mid_recorded = false;
    std::vector<TextureImpl*> tail_reads, tail_writes;
    size_t sync_used = 0;
    std::vector<Op> ops;
    bool submitted = false;
    GPU_ComputePipeline* bound_cpipe = nullptr;
    GPU_DescriptorSet* bound_cset = nullptr;
    uint8_t push[128]; uint32_t push_size = 0;
    GPU_RenderPass* preparing = nullptr; GPU_RenderPass* in_pass = nullptr;
    std::vector<DrawParams> draw_params;
    int bound_draw = -1;
    BufferImpl* vertex_buffer = nullptr; BufferImpl* index_buffer = nullptr;     // GPU_OpBindVertexBuffer / GPU_OpBindIndexBuffer
    int raster_op = -1;                            // index in ops of the raster job of the open render pass (-1: none yet)
    std::vector<RasterScratch> raster; size_t raster_used = 0;
    void* sh_scratch = nullptr; size_t sh_scratch_bytes = 0;   // K17 partials (GPUX_OpProjectSH9): sized at record time, kept across submissions
    // K20 / K21 / K22 tables (GPUX_OpCubeToPanorama, GPUX_OpPrefilterGGX, GPUX_OpBrdfLutGGX), one per recorded op: allocated and filled at record time, handed out again after a reset
    // (a table that is big enough is kept), freed with the graph
    struct PanoTable { void* dev = nullptr; size_t bytes = 0; };
    std::vector<PanoTable> pano; size_t pano_used = 0;
    // hipGraph replay (GPUX_SetGraphReplay): the executable graph of the previous submission, updated in place when the
    // next one has the same shape
    hipGraphExec_t exec = nullptr;
    bool replay_broken = false;                    // a capture failed on this graph: it stays on plain launches
    uint64_t replay_launches = 0, replay_updates = 0, replay_instantiations = 0;
    // Which kernel each lighting op of the submission launches (5: K5, 16: K16 -- decided at execution time from the Globals), and the
    // same for the submission `exec` was instantiated from.  hipGraphExecUpdate is not relied upon to notice a changed kernel function:
    // when the two differ, the executable graph is destroyed and instantiated anew.
    std::vector<uint8_t> launch_sig, exec_sig;
    // timing of the last waited submission
    std::vector<hipEvent_t> ev;
    std::vector<std::string> timed_names;
    std::vector<float> timed_ms;
    // one event pair on the graph's main stream around the whole submission (first op start .. last join): the busy span of the
    // graph's kernels even when its dispatches overlap on side streams (the sum of per-op times would count the overlap twice)
    hipEvent_t span_a = nullptr, span_b = nullptr;
    bool span_recorded = false;
    float span_ms = 0.0f;
};

struct DeviceTable { void* dev = nullptr; int count = 0; float alpha = 0.0f; std::vector<float> weights; /* prefilter tables: w_i of the kept entries, in order */ };
struct TableKey {
    int kind, n, aux; uint32_t rbits;
    bool operator<(const TableKey& o) const {
        if (kind != o.kind) return kind < o.kind;
        if (n != o.n) return n < o.n;
        if (aux != o.aux) return aux < o.aux;
        return rbits < o.rbits;
    }
};

static struct {
    GPU_Graph* last_submitted = nullptr;            // submission order between graphs (the reference has one queue: gpu_vulkan.c:2481)
    bool init = false;
    int device = -1;
    GPU_Sampler samplers[6];
    std::map<TableKey, DeviceTable> tables;
    bool timing = false;
    float prefilter_tol = 0.0f;                     // GPUX_SetPrefilterTolerance: 0 = exact sums (default)
    int kept_samples[32] = {0};                     // per output mip: samples kept by the last prefilter dispatch
    // submit-time settings, each read once on first use (env_setting; -1: not read yet) unless its GPUX_Set* call came first
    int fold = -1;                                  // PBR_GRAPH_FOLD or 1: fold_blits
    int order = -1;                                 // PBR_GRAPH_ORDER or 1; 0: diagnostic only (shows that the ordering test can fail)
    int overlap = -1;                               // GPUX_SetGraphOverlap, PBR_GRAPH_OVERLAP or 1: head / tail overlap of frames in flight
    int replay = -1;                                // GPUX_SetGraphReplay, PBR_GRAPH_REPLAY or 0: submissions go through an instantiated hipGraph
    int tile_streams = -1;                          // GPUX_SetTileStreams, PBR_TILE_STREAMS or 4: side streams for small independent precompute dispatches
    int level_overlap = 1;                          // GPUX_SetLevelOverlap: independent whole levels of a submission run side by side (TileRegion)
    int level_streams = -1;                         // GPUX_SetLevelStreams, or kLevelStreams: the streams they are spread over
    unsigned long long* raster_rejected = nullptr;  // device counters: [0] GPUX_RasterRejectedTriangles, [1] GPUX_VoxelizeFragments
    uint64_t raster_rejected_base = 0;              // what earlier GPU_Init .. GPU_Deinit spans counted
} G;

static const int kLevelStreams = 2;                 // the only count that gained on all three bench workloads: profiles/level_streams.md
static const char kTokenLut[] = "HIPK1:gen_brdf_integration_map";
static const char kTokenIrr[] = "HIPK3:gen_irradiance_map";
static const char kTokenPre[] = "HIPK4:gen_prefiltered_env_map";
static const char kTokenLit[] = "HIPK5:lighting_pass";
static const char kTokenSweep[] = "HIPK7:lightgrid_sweep";
static const char kTokenTaa[] = "HIPK8:taa_resolve";
static const char kTokenFinal[] = "HIPK9:final_post_process";
static const char kTokenBloomDown[] = "HIPK10:bloom_downsample";
static const char kTokenBloomUp[] = "HIPK11:bloom_upsample";
static const char kTokenSun[] = "HIPK12:sun_depth_pass";
static const char kTokenGeometry[] = "HIPK13:geometry_pass";
static const char kTokenVoxelize[] = "HIPK14:lightgrid_voxelize";

// ------------------------------------------------------------------------------------------
// formats  [gpu.h:99-144]
// ------------------------------------------------------------------------------------------
GPU_API GPU_FormatInfo GPUX_GetFormatInfo(GPU_Format f) {
    struct Row { GPU_Format f; uint32_t ext, size; bool s, v, c, d, st, i; const char* glsl; };
    static const Row rows[] = {
        {GPU_Format_R8UN, 1, 1, 1, 1, 1, 0, 0, 0, "r8"}, {GPU_Format_RG8UN, 1, 2, 1, 1, 1, 0, 0, 0, "rg8"},
        {GPU_Format_RGBA8UN, 1, 4, 1, 1, 1, 0, 0, 0, "rgba8"}, {GPU_Format_BGRA8UN, 1, 4, 1, 1, 1, 0, 0, 0, nullptr},
        {GPU_Format_R16F, 1, 2, 1, 1, 1, 0, 0, 0, "r16f"}, {GPU_Format_RG16F, 1, 4, 1, 1, 1, 0, 0, 0, "rg16f"},
        {GPU_Format_RGB16F, 1, 6, 0, 1, 0, 0, 0, 0, nullptr}, {GPU_Format_RGBA16F, 1, 8, 1, 1, 1, 0, 0, 0, "rgba16f"},
        {GPU_Format_R32F, 1, 4, 1, 1, 1, 0, 0, 0, "r32f"}, {GPU_Format_RG32F, 1, 8, 1, 1, 1, 0, 0, 0, "rg32f"},
        {GPU_Format_RGB32F, 1, 12, 0, 1, 0, 0, 0, 0, nullptr}, {GPU_Format_RGBA32F, 1, 16, 1, 1, 1, 0, 0, 0, "rgba32f"},
        {GPU_Format_R8I, 1, 1, 1, 1, 1, 0, 0, 1, "r8ui"}, {GPU_Format_R16I, 1, 2, 1, 1, 1, 0, 0, 1, "r16ui"},
        {GPU_Format_RG16I, 1, 4, 1, 1, 1, 0, 0, 1, "rg16ui"}, {GPU_Format_RGBA16I, 1, 8, 1, 1, 1, 0, 0, 1, "rgba16ui"},
        {GPU_Format_R32I, 1, 4, 1, 1, 1, 0, 0, 1, "r32ui"}, {GPU_Format_RG32I, 1, 8, 1, 1, 1, 0, 0, 1, "rg32ui"},
        {GPU_Format_RGB32I, 1, 12, 1, 1, 0, 0, 0, 1, nullptr}, {GPU_Format_RGBA32I, 1, 16, 1, 1, 1, 0, 0, 1, "rgba32ui"},
        {GPU_Format_R64I, 1, 8, 0, 0, 0, 0, 0, 1, "r64ui"}, {GPU_Format_D16UN, 1, 2, 1, 0, 0, 1, 0, 0, nullptr},
        {GPU_Format_D32F_Or_X8D24UN, 1, 4, 1, 0, 0, 1, 0, 0, nullptr}, {GPU_Format_D32FS8I_Or_D24UNS8I, 1, 5, 0, 0, 0, 1, 0, 0, nullptr},
        {GPU_Format_D24UNS8I_Or_D32FS8I, 1, 4, 0, 0, 0, 1, 0, 0, nullptr},
        {GPU_Format_BC1_RGB_UN, 4, 8, 1, 0, 0, 0, 0, 0, nullptr}, {GPU_Format_BC1_RGBA_UN, 4, 8, 1, 0, 0, 0, 0, 0, nullptr},
        {GPU_Format_BC3_RGBA_UN, 4, 16, 1, 0, 0, 0, 0, 0, nullptr}, {GPU_Format_BC5_UN, 4, 16, 1, 0, 0, 0, 0, 0, nullptr},
    };
    for (const Row& r : rows)
        if (r.f == f) { GPU_FormatInfo o = {r.ext, r.size, r.s, r.v, r.c, r.d, r.st, r.i, r.glsl}; return o; }
    GPU_FormatInfo z = {0, 0, false, false, false, false, false, false, nullptr};
    return z;
}

// ------------------------------------------------------------------------------------------
// lifetime
// ------------------------------------------------------------------------------------------
GPU_API void GPUX_SetDevice(int idx) { G.device = idx; }
GPU_API int GPUX_GetDevice(void) { return G.device; }
GPU_API void GPUX_SetErrorHandler(GPUX_ErrorHandler h, void* user) { g_err_handler = h; g_err_user = user; }
GPU_API const char* GPUX_BackendName(void) { return "hip-gfx950"; }

static void make_shared_sampler(GPU_Sampler* s, GPU_Filter f, GPU_AddressMode m) {
    memset(&s->desc, 0, sizeof s->desc);
    s->desc.min_filter = s->desc.mag_filter = s->desc.mipmap_mode = f;     // gpu_vulkan.c:935-943
    s->desc.address_modes[0] = s->desc.address_modes[1] = s->desc.address_modes[2] = m;
    s->desc.max_lod = 1000.0f;
    s->shared = true;
}

GPU_API void GPU_Init(GPU_WindowHandle window) {
    (void)window;   // headless
    GPU_REQUIRE_V(!G.init, "GPU_Init: already initialised");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    GPU_REQUIRE_V(e == hipSuccess && count > 0, "GPU_Init: no HIP device (%s)", hipGetErrorString(e));
    if (G.device < 0) {
        const char* lr = getenv("LOCAL_RANK");
        G.device = lr ? atoi(lr) % count : 0;
    }
    GPU_REQUIRE_V(G.device < count, "GPU_Init: device %d out of range (%d devices)", G.device, count);
    HIP_OK(hipSetDevice(G.device));
    make_shared_sampler(&G.samplers[0], GPU_Filter_Linear, GPU_AddressMode_Wrap);
    make_shared_sampler(&G.samplers[1], GPU_Filter_Linear, GPU_AddressMode_Clamp);
    make_shared_sampler(&G.samplers[2], GPU_Filter_Linear, GPU_AddressMode_Mirror);
    make_shared_sampler(&G.samplers[3], GPU_Filter_Nearest, GPU_AddressMode_Clamp);
    make_shared_sampler(&G.samplers[4], GPU_Filter_Nearest, GPU_AddressMode_Wrap);
    make_shared_sampler(&G.samplers[5], GPU_Filter_Nearest, GPU_AddressMode_Mirror);
    G.init = true;
}

GPU_API void GPU_Deinit(void) {
    if (!G.init) return;
    (void)hipDeviceSynchronize();
    pbrk_mc_bin_cache_clear();                                  // the bin cache's buffers go with the tables they were recorded from
    for (auto& kv : G.tables) { (void)pbrk_mc_table_unregister(kv.second.dev); (void)hipFree(kv.second.dev); }
    G.tables.clear();
    if (G.raster_rejected) {
        unsigned long long d = 0;
        if (hipMemcpy(&d, G.raster_rejected, 8, hipMemcpyDeviceToHost) == hipSuccess) G.raster_rejected_base += d;
        (void)hipFree(G.raster_rejected); G.raster_rejected = nullptr;
    }
    G.init = false;
}

GPU_API void GPU_WaitUntilIdle(void) { if (G.init) HIP_OK(hipDeviceSynchronize()); }

// ------------------------------------------------------------------------------------------
// samplers
// ------------------------------------------------------------------------------------------
GPU_API GPU_Sampler* GPU_SamplerLinearWrap(void) { return &G.samplers[0]; }
GPU_API GPU_Sampler* GPU_SamplerLinearClamp(void) { return &G.samplers[1]; }
GPU_API GPU_Sampler* GPU_SamplerLinearMirror(void) { return &G.samplers[2]; }
GPU_API GPU_Sampler* GPU_SamplerNearestClamp(void) { return &G.samplers[3]; }
GPU_API GPU_Sampler* GPU_SamplerNearestWrap(void) { return &G.samplers[4]; }
GPU_API GPU_Sampler* GPU_SamplerNearestMirror(void) { return &G.samplers[5]; }
GPU_API GPU_Sampler* GPU_MakeSampler(const GPU_SamplerDesc* desc) {
    GPU_REQUIRE(desc, nullptr, "GPU_MakeSampler: desc is NULL");
    GPU_Sampler* s = new GPU_Sampler();
    s->desc = *desc; s->shared = false;
    return s;
}
GPU_API void GPU_DestroySampler(GPU_Sampler* s) {
    if (!s) return;
    GPU_REQUIRE_V(!s->shared, "GPU_DestroySampler: shared sampler shortcuts must not be destroyed");
    delete s;
}

// ------------------------------------------------------------------------------------------
// pipeline layouts
// ------------------------------------------------------------------------------------------
GPU_API GPU_PipelineLayout* GPU_InitPipelineLayout(void) { return new GPU_PipelineLayout(); }
static GPU_Binding add_binding(GPU_PipelineLayout* l, const char* name, BindKind k, GPU_Format f, const char* fn) {
    GPU_REQUIRE(l && name, 0, "%s: NULL argument", fn);
    GPU_REQUIRE(!l->finalized, 0, "%s: layout already finalised", fn);
    l->bindings.push_back({name, k, f});
    return (GPU_Binding)(l->bindings.size() - 1);
}
GPU_API GPU_Binding GPU_TextureBinding(GPU_PipelineLayout* l, const char* name) { return add_binding(l, name, Bind_Texture, GPU_Format_Invalid, __func__); }
GPU_API GPU_Binding GPU_SamplerBinding(GPU_PipelineLayout* l, const char* name) { return add_binding(l, name, Bind_Sampler, GPU_Format_Invalid, __func__); }
GPU_API GPU_Binding GPU_BufferBinding(GPU_PipelineLayout* l, const char* name) { return add_binding(l, name, Bind_Buffer, GPU_Format_Invalid, __func__); }
GPU_API GPU_Binding GPU_StorageImageBinding(GPU_PipelineLayout* l, const char* name, GPU_Format f) { return add_binding(l, name, Bind_StorageImage, f, __func__); }
GPU_API void GPU_FinalizePipelineLayout(GPU_PipelineLayout* l) {
    GPU_REQUIRE_V(l, "GPU_FinalizePipelineLayout: NULL layout");
    l->finalized = true;
}
GPU_API void GPU_DestroyPipelineLayout(GPU_PipelineLayout* l) { delete l; }

static int find_binding(const GPU_PipelineLayout* l, const char* name) {
    for (size_t i = 0; i < l->bindings.size(); ++i) if (l->bindings[i].name == name) return (int)i;
    return -1;
}
static Slot* named_slot(GPU_DescriptorSet* set, const char* name) {
    int b = find_binding(set->layout, name);
    return b < 0 ? nullptr : &set->slots[b];
}

// ------------------------------------------------------------------------------------------
// descriptor sets
// ------------------------------------------------------------------------------------------
GPU_API GPU_DescriptorArena* GPU_MakeDescriptorArena(void) { return new GPU_DescriptorArena(); }
GPU_API void GPU_ResetDescriptorArena(GPU_DescriptorArena* a) {
    GPU_REQUIRE_V(a, "GPU_ResetDescriptorArena: NULL arena");
    for (GPU_DescriptorSet* s : a->sets) delete s;
    a->sets.clear();
}
GPU_API void GPU_DestroyDescriptorArena(GPU_DescriptorArena* a) {
    if (!a) return;
    for (GPU_DescriptorSet* s : a->sets) delete s;
    delete a;
}
GPU_API GPU_DescriptorSet* GPU_InitDescriptorSet(GPU_DescriptorArena* arena, GPU_PipelineLayout* layout) {
    GPU_REQUIRE(layout && layout->finalized, nullptr, "GPU_InitDescriptorSet: layout is NULL or not finalised");
    GPU_DescriptorSet* s = new GPU_DescriptorSet();
    s->layout = layout;
    s->slots.resize(layout->bindings.size());
    for (size_t i = 0; i < s->slots.size(); ++i) s->slots[i].kind = layout->bindings[i].kind;
    s->arena = arena;
    if (arena) arena->sets.push_back(s);
    return s;
}
static Slot* slot_for(GPU_DescriptorSet* set, GPU_Binding b, BindKind kind, const char* fn) {
    GPU_REQUIRE(set, nullptr, "%s: NULL descriptor set", fn);
    GPU_REQUIRE(!set->finalized, nullptr, "%s: descriptor set already finalised", fn);
    GPU_REQUIRE(b < set->slots.size(), nullptr, "%s: binding %u out of range", fn, b);
    GPU_REQUIRE(set->slots[b].kind == kind, nullptr, "%s: binding %u (\"%s\") has a different kind", fn, b, set->layout->bindings[b].name.c_str());
    return &set->slots[b];
}
GPU_API void GPU_SetTextureBinding(GPU_DescriptorSet* set, GPU_Binding b, GPU_Texture* v) {
    Slot* s = slot_for(set, b, Bind_Texture, __func__); if (!s) return;
    GPU_REQUIRE_V(v, "GPU_SetTextureBinding: NULL texture");
    s->tex = (TextureImpl*)v; s->whole = true; s->mip = 0; s->set = true;
}
GPU_API void GPU_SetTextureMipBinding(GPU_DescriptorSet* set, GPU_Binding b, GPU_Texture* v, uint32_t mip) {
    Slot* s = slot_for(set, b, Bind_Texture, __func__); if (!s) return;
    GPU_REQUIRE_V(v && mip < v->mip_level_count, "GPU_SetTextureMipBinding: bad texture / mip");
    GPU_REQUIRE_V(v->flags & GPU_TextureFlag_PerMipBinding, "GPU_SetTextureMipBinding: texture lacks GPU_TextureFlag_PerMipBinding");
    s->tex = (TextureImpl*)v; s->whole = false; s->mip = mip; s->set = true;
}
GPU_API void GPU_SetSamplerBinding(GPU_DescriptorSet* set, GPU_Binding b, GPU_Sampler* v) {
    Slot* s = slot_for(set, b, Bind_Sampler, __func__); if (!s) return;
    GPU_REQUIRE_V(v, "GPU_SetSamplerBinding: NULL sampler");
    s->sampler = v; s->set = true;
}
GPU_API void GPU_SetBufferBinding(GPU_DescriptorSet* set, GPU_Binding b, GPU_Buffer* v) {
    Slot* s = slot_for(set, b, Bind_Buffer, __func__); if (!s) return;
    GPU_REQUIRE_V(v, "GPU_SetBufferBinding: NULL buffer");
    s->buf = (BufferImpl*)v; s->set = true;
}
GPU_API void GPU_SetStorageImageBinding(GPU_DescriptorSet* set, GPU_Binding b, GPU_Texture* v, uint32_t mip) {
    Slot* s = slot_for(set, b, Bind_StorageImage, __func__); if (!s) return;
    GPU_REQUIRE_V(v && mip < v->mip_level_count, "GPU_SetStorageImageBinding: bad texture / mip level %u", mip);
    GPU_REQUIRE_V(v->flags & GPU_TextureFlag_StorageImage, "GPU_SetStorageImageBinding: texture lacks GPU_TextureFlag_StorageImage");
    s->tex = (TextureImpl*)v; s->whole = false; s->mip = mip; s->set = true;
}
GPU_API void GPU_FinalizeDescriptorSet(GPU_DescriptorSet* set) {
    GPU_REQUIRE_V(set, "GPU_FinalizeDescriptorSet: NULL set");
    for (size_t i = 0; i < set->slots.size(); ++i)
        GPU_REQUIRE_V(set->slots[i].set, "GPU_FinalizeDescriptorSet: binding %zu (\"%s\") was never set", i, set->layout->bindings[i].name.c_str());
    set->finalized = true;
}
GPU_API void GPU_DestroyDescriptorSet(GPU_DescriptorSet* set) {
    if (!set) return;
    GPU_REQUIRE_V(!set->arena, "GPU_DestroyDescriptorSet: set belongs to an arena");
    delete set;
}

// ------------------------------------------------------------------------------------------
// resources
// ------------------------------------------------------------------------------------------
static inline uint32_t mip_dim(uint32_t d, uint32_t m) { uint32_t v = d >> m; return v < 1 ? 1 : v; }

GPU_API uint64_t GPUX_TextureMipBytes(const GPU_Texture* t, uint32_t mip) {
    if (!t || mip >= t->mip_level_count) return 0;
    GPU_FormatInfo fi = GPUX_GetFormatInfo(t->format);
    uint64_t w = mip_dim(t->width, mip), h = mip_dim(t->height, mip), d = mip_dim(t->depth, mip);
    uint64_t bw = (w + fi.block_extent - 1) / fi.block_extent, bh = (h + fi.block_extent - 1) / fi.block_extent;
    return bw * bh * d * fi.block_size * t->layer_count;
}

// 2-D RGBA8UN with power-of-two extents: the material textures of the geometry pass (K13)
static bool is_rgba8_pow2(const TextureImpl* t) {
    const uint32_t w = t->base.width, h = t->base.height;
    return t->base.format == GPU_Format_RGBA8UN && t->base.layer_count == 1 && t->base.depth == 1 && (w & (w - 1)) == 0 && (h & (h - 1)) == 0;
}
// K15: the block-compressed formats and their decoded twin
static int bc_kernel_format(GPU_Format f) {
    switch (f) {
    case GPU_Format_BC1_RGB_UN: return PBRK_BC1_RGB;
    case GPU_Format_BC1_RGBA_UN: return PBRK_BC1_RGBA;
    case GPU_Format_BC3_RGBA_UN: return PBRK_BC3;
    case GPU_Format_BC5_UN: return PBRK_BC5;
    default: return -1;
    }
}
static bool is_bc_format(GPU_Format f) { return bc_kernel_format(f) >= 0; }
// what the material slots of K13 / K14 accept: a 2-D one-layer RGBA8UN texture, or a BC texture that carries a decoded image
static bool is_material_2d(const TextureImpl* t) {
    if (t->base.layer_count != 1 || t->base.depth != 1) return false;
    return t->base.format == GPU_Format_RGBA8UN || (is_bc_format(t->base.format) && t->decoded);
}
static const void* material_texels(const TextureImpl* t) { return t->decoded ? t->decoded : t->dev; }
// decode one level of a BC texture from its blocks into the decoded image, on `st`
static int decode_bc_level(TextureImpl* t, uint32_t mip, hipStream_t st) {
    return pbrk_bc_decode(bc_kernel_format(t->base.format), (const char*)t->dev + t->mip_offset[mip], (int)mip_dim(t->base.width, mip),
                          (int)mip_dim(t->base.height, mip), (char*)t->decoded + t->decoded_offset[mip], st);
}
static bool is_f4_cube(const TextureImpl* t) {
    return t->base.format == GPU_Format_RGBA32F && (t->base.flags & GPU_TextureFlag_Cubemap) && t->base.width == t->base.height && t->base.depth == 1;
}

static GPU_Texture* make_texture_impl(GPU_Format format, uint32_t width, uint32_t height, uint32_t depth, GPU_TextureFlags flags,
                                      const void* data, void* external, uint64_t external_bytes, const char* fn) {
    GPU_REQUIRE(G.init, nullptr, "%s: GPU_Init has not been called", fn);
    GPU_REQUIRE(width > 0 && height > 0 && depth > 0, nullptr, "%s: zero extent", fn);   // gpu_vulkan.c:1339
    GPU_FormatInfo fi = GPUX_GetFormatInfo(format);
    GPU_REQUIRE(fi.block_size > 0, nullptr, "%s: invalid format %d", fn, (int)format);
    const bool bc = is_bc_format(format);
    // a compressed chain cannot be generated (and the reference never asks for one): levels of a BC texture arrive by copies
    GPU_REQUIRE(!(bc && data && (flags & GPU_TextureFlag_HasMipmaps)), nullptr,
                "%s: GPU_TextureFlag_HasMipmaps with data is not supported for block-compressed formats (create the texture without data and copy every level in)", fn);
    GPU_REQUIRE(!(bc && (width > 16384 || height > 16384)), nullptr, "%s: block-compressed textures are limited to 16384 x 16384", fn);
    TextureImpl* t = new TextureImpl();
    t->base.width = width; t->base.height = height; t->base.depth = depth;
    t->base.layer_count = (flags & GPU_TextureFlag_Cubemap) ? 6 : 1;
    uint32_t mips = 1;
    if (flags & GPU_TextureFlag_HasMipmaps) {                                  // gpu_vulkan.c:1344-1351
        uint32_t s = width < height ? width : height;
        while (s > 1) { s /= 2; mips++; }
    }
    t->base.mip_level_count = mips;
    t->base.format = format; t->base.flags = flags;
    t->texel_bytes = fi.block_size;
    size_t off = 0;
    for (uint32_t m = 0; m < mips; ++m) { t->mip_offset.push_back(off); off += (size_t)GPUX_TextureMipBytes(&t->base, m); }
    t->bytes = off;
    if (external) {
        if (external_bytes < t->bytes) { gpu_fail("%s: external allocation of %llu bytes is smaller than the %zu the texture needs", fn, (unsigned long long)external_bytes, t->bytes); delete t; return nullptr; }
        t->dev = external; t->owns_memory = false;
    } else {
        hipError_t e = hipMalloc(&t->dev, t->bytes);
        if (e != hipSuccess) { gpu_fail("%s: hipMalloc(%zu) failed: %s", fn, t->bytes, hipGetErrorString(e)); delete t; return nullptr; }
        HIP_OK(hipMemset(t->dev, 0, t->bytes));
    }
    if (bc && t->base.layer_count == 1 && depth == 1) {                        // K15: the decoded image the draws sample
        size_t doff = 0;
        for (uint32_t m = 0; m < mips; ++m) { t->decoded_offset.push_back(doff); doff += (size_t)mip_dim(width, m) * mip_dim(height, m) * 4; }
        hipError_t e = hipMalloc(&t->decoded, doff);
        if (e != hipSuccess) { gpu_fail("%s: hipMalloc(%zu) for the decoded image failed: %s", fn, doff, hipGetErrorString(e)); t->decoded = nullptr; GPU_DestroyTexture(&t->base); return nullptr; }
        HIP_OK(hipMemset(t->decoded, 0, doff));
    }
    if (data) {
        HIP_OK(hipMemcpy(t->dev, data, (size_t)GPUX_TextureMipBytes(&t->base, 0), hipMemcpyHostToDevice));
        if (t->decoded) {                                                      // level 0 is decoded before the call returns
            int rc = decode_bc_level(t, 0, nullptr);
            if (rc != PBRK_OK) gpu_fail("%s: K15 launch failed (%d)", fn, rc);
            HIP_OK(hipStreamSynchronize(nullptr));
        }
        if (mips > 1) {                                                        // gpu_vulkan.c:1444-1446
            if (is_rgba8_pow2(t)) {
                int rc = pbrk_mip_chain_rgba8(t->dev, (int)width, (int)height, (int)mips, nullptr);
                if (rc != PBRK_OK) gpu_fail("%s: RGBA8UN mip chain kernel failed (%d)", fn, rc);
                HIP_OK(hipStreamSynchronize(nullptr));
            } else if (!is_f4_cube(t)) {
                gpu_fail("%s: mip generation is implemented for RGBA32F cubemaps and power-of-two 2-D RGBA8UN textures only", fn);
            } else {
                int rc = pbrk_mip_chain(t->dev, (int)width, (int)mips, nullptr);
                if (rc != PBRK_OK) gpu_fail("%s: mip chain kernel failed (%d)", fn, rc);
                HIP_OK(hipStreamSynchronize(nullptr));                          // :1448-1449 blocking
            }
        }
    }
    return &t->base;
}

GPU_API GPU_Texture* GPU_MakeTexture(GPU_Format format, uint32_t width, uint32_t height, uint32_t depth, GPU_TextureFlags flags, const void* data) {
    return make_texture_impl(format, width, height, depth, flags, data, nullptr, 0, __func__);
}
GPU_API GPU_Texture* GPUX_MakeTextureExternal(GPU_Format format, uint32_t width, uint32_t height, uint32_t depth, GPU_TextureFlags flags,
                                              void* device_memory, uint64_t device_bytes) {
    GPU_REQUIRE(device_memory, nullptr, "GPUX_MakeTextureExternal: NULL device memory");
    return make_texture_impl(format, width, height, depth, flags, nullptr, device_memory, device_bytes, __func__);
}
GPU_API GPU_Texture* GPUX_MakeCubemapFromEquirect(const void* rgba32f, uint32_t width, uint32_t height, uint32_t face_size, GPU_TextureFlags extra_flags) {
    GPU_REQUIRE(rgba32f && width > 0 && height > 0 && face_size > 0, nullptr, "GPUX_MakeCubemapFromEquirect: bad arguments");
    GPU_Texture* tex = make_texture_impl(GPU_Format_RGBA32F, face_size, face_size, 1, GPU_TextureFlag_Cubemap | GPU_TextureFlag_HasMipmaps | extra_flags,
                                         nullptr, nullptr, 0, __func__);
    if (!tex) return nullptr;
    TextureImpl* t = (TextureImpl*)tex;
    void* pano = nullptr;
    size_t bytes = (size_t)width * height * 16;
    hipError_t e = hipMalloc(&pano, bytes);
    if (e != hipSuccess) { gpu_fail("GPUX_MakeCubemapFromEquirect: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); GPU_DestroyTexture(tex); return nullptr; }
    HIP_OK(hipMemcpy(pano, rgba32f, bytes, hipMemcpyHostToDevice));
    int rc = pbrk_equirect_to_cube(pano, (int)width, (int)height, t->dev, (int)face_size, nullptr);
    if (rc == PBRK_OK) rc = pbrk_mip_chain(t->dev, (int)face_size, (int)tex->mip_level_count, nullptr);
    HIP_OK(hipStreamSynchronize(nullptr));
    (void)hipFree(pano);
    if (rc != PBRK_OK) { gpu_fail("GPUX_MakeCubemapFromEquirect: conversion kernels failed (%d)", rc); GPU_DestroyTexture(tex); return nullptr; }
    return tex;
}
GPU_API uint64_t GPUX_TextureTotalBytes(const GPU_Texture* t) { return t ? ((const TextureImpl*)t)->bytes : 0; }
GPU_API uint64_t GPUX_TextureMipOffset(const GPU_Texture* t, uint32_t mip) {
    return (t && mip < t->mip_level_count) ? ((const TextureImpl*)t)->mip_offset[mip] : 0;
}

GPU_API void GPU_DestroyTexture(GPU_Texture* tex) {
    if (!tex) return;
    TextureImpl* t = (TextureImpl*)tex;
    if (t->owns_memory) (void)hipFree(t->dev);
    free_derived(t);
    if (t->decoded) (void)hipFree(t->decoded);
    delete t;
}

GPU_API GPU_Buffer* GPU_MakeBuffer(uint32_t size, GPU_BufferFlags flags, const void* data) {
    GPU_REQUIRE(G.init, nullptr, "GPU_MakeBuffer: GPU_Init has not been called");
    GPU_REQUIRE(size > 0, nullptr, "GPU_MakeBuffer: zero size");
    BufferImpl* b = new BufferImpl();
    b->base.flags = flags; b->base.size = size; b->base.data = nullptr;
    hipError_t e;
    if (flags & GPU_BufferFlag_CPU) {                                          // persistently mapped (gpu_vulkan.c:1248-1250)
        e = hipHostMalloc(&b->dev, size, hipHostMallocDefault);
        b->pinned_host = true;
        b->base.data = b->dev;
    } else {
        e = hipMalloc(&b->dev, size);
    }
    if (e != hipSuccess) { gpu_fail("GPU_MakeBuffer: allocation of %u bytes failed: %s", size, hipGetErrorString(e)); delete b; return nullptr; }
    if (data) {
        if (b->pinned_host) memcpy(b->dev, data, size);
        else HIP_OK(hipMemcpy(b->dev, data, size, hipMemcpyHostToDevice));
    }
    return &b->base;
}

GPU_API void GPU_DestroyBuffer(GPU_Buffer* buf) {
    if (!buf) return;
    BufferImpl* b = (BufferImpl*)buf;
    if (b->pinned_host) (void)hipHostFree(b->dev); else (void)hipFree(b->dev);
    delete b;
}

GPU_API void* GPUX_TextureDevicePtr(GPU_Texture* tex, uint32_t mip) {
    GPU_REQUIRE(tex && mip < tex->mip_level_count, nullptr, "GPUX_TextureDevicePtr: bad texture / mip");
    TextureImpl* t = (TextureImpl*)tex;
    return (char*)t->dev + t->mip_offset[mip];
}
GPU_API void GPUX_InvalidateTexture(GPU_Texture* tex) {
    GPU_REQUIRE_V(tex, "GPUX_InvalidateTexture: NULL texture");
    texture_written((TextureImpl*)tex);
}
GPU_API void* GPUX_BufferDevicePtr(GPU_Buffer* buf) { return buf ? ((BufferImpl*)buf)->dev : nullptr; }

// ------------------------------------------------------------------------------------------
// pipelines: shader identity -> built-in kernel
// ------------------------------------------------------------------------------------------
static std::string basename_of(GPU_String path) {
    std::string s(path.data ? path.data : "", path.data ? path.length : 0);
    size_t p = s.find_last_of("/\\");
    return p == std::string::npos ? s : s.substr(p + 1);
}
static bool glsl_contains(GPU_String glsl, const char* needle) {
    if (!glsl.data || glsl.length == 0) return true;        // no text given: trust the file name
    std::string s(glsl.data, glsl.length);
    return s.find(needle) != std::string::npos;
}
static KernelId identify_shader(const GPU_ShaderDesc* d) {
    if (d->spirv.data && d->spirv.length) {
        std::string t(d->spirv.data, d->spirv.length);
        if (t == kTokenLut) return Kernel_BrdfLut;
        if (t == kTokenIrr) return Kernel_Irradiance;
        if (t == kTokenPre) return Kernel_Prefilter;
        if (t == kTokenLit) return Kernel_Lighting;
        if (t == kTokenSweep) return Kernel_LightgridSweep;
        if (t == kTokenTaa) return Kernel_TaaResolve;
        if (t == kTokenFinal) return Kernel_FinalPost;
        if (t == kTokenBloomDown) return Kernel_BloomDown;
        if (t == kTokenBloomUp) return Kernel_BloomUp;
        if (t == kTokenSun) return Kernel_SunDepth;
        if (t == kTokenGeometry) return Kernel_Geometry;
        if (t == kTokenVoxelize) return Kernel_Voxelize;
        return Kernel_None;
    }
    std::string b = basename_of(d->glsl_debug_filepath);
    // file name first; the GLSL text (when present) must carry the entry's signature symbols
    if (b == "gen_brdf_integration_map.glsl" && glsl_contains(d->glsl, "GeometryMikkelsen") && glsl_contains(d->glsl, "image2D OUTPUT")) return Kernel_BrdfLut;
    if (b == "gen_irradiance_map.glsl" && glsl_contains(d->glsl, "CubemapSampleDirFromFaceUV") && glsl_contains(d->glsl, "TEX_ENV_CUBE")) return Kernel_Irradiance;
    if (b == "gen_prefiltered_env_map.glsl" && glsl_contains(d->glsl, "DistributionBeckmann") && glsl_contains(d->glsl, "mip_level")) return Kernel_Prefilter;
    if (b == "lighting_pass.glsl" && glsl_contains(d->glsl, "BRDF_INTEGRATION_MAP") && glsl_contains(d->glsl, "GBUFFER_DEPTH")) return Kernel_Lighting;
    if (b == "taa_resolve.glsl" && glsl_contains(d->glsl, "SampleHistoryTextureCatmullRom") && glsl_contains(d->glsl, "GBUFFER_VELOCITY_PREV")) return Kernel_TaaResolve;
    if (b == "final_post_process.glsl" && glsl_contains(d->glsl, "aces_approx") && glsl_contains(d->glsl, "BLOOM_RESULT")) return Kernel_FinalPost;
    if (b == "bloom_downsample.glsl" && glsl_contains(d->glsl, "BLOOM_INPUT") && glsl_contains(d->glsl, "dst_mip_level")) return Kernel_BloomDown;
    if (b == "bloom_upsample.glsl" && glsl_contains(d->glsl, "BLOOM_INPUT") && glsl_contains(d->glsl, "radius")) return Kernel_BloomUp;
    if (b == "lightgrid_sweep.glsl" && glsl_contains(d->glsl, "LIGHTMAP_IMG") && glsl_contains(d->glsl, "X_direction")) return Kernel_LightgridSweep;
    if (b == "sun_depth_pass.glsl" && glsl_contains(d->glsl, "sun_space_from_world") && glsl_contains(d->glsl, "vs_position")) return Kernel_SunDepth;
    if (b == "geometry_pass.glsl" && glsl_contains(d->glsl, "old_clip_space_from_world") && glsl_contains(d->glsl, "out_velocity")) return Kernel_Geometry;
    if (b == "lightgrid_voxelize.glsl" && glsl_contains(d->glsl, "LIGHTMAP_IMG") && glsl_contains(d->glsl, "lightgrid_scale")) return Kernel_Voxelize;
    return Kernel_None;
}
static GPU_String token_for(KernelId k) {
    switch (k) {
    case Kernel_BrdfLut: return GPU_String{kTokenLut, sizeof kTokenLut - 1};
    case Kernel_Irradiance: return GPU_String{kTokenIrr, sizeof kTokenIrr - 1};
    case Kernel_Prefilter: return GPU_String{kTokenPre, sizeof kTokenPre - 1};
    case Kernel_Lighting: return GPU_String{kTokenLit, sizeof kTokenLit - 1};
    case Kernel_LightgridSweep: return GPU_String{kTokenSweep, sizeof kTokenSweep - 1};
    case Kernel_TaaResolve: return GPU_String{kTokenTaa, sizeof kTokenTaa - 1};
    case Kernel_FinalPost: return GPU_String{kTokenFinal, sizeof kTokenFinal - 1};
    case Kernel_BloomDown: return GPU_String{kTokenBloomDown, sizeof kTokenBloomDown - 1};
    case Kernel_BloomUp: return GPU_String{kTokenBloomUp, sizeof kTokenBloomUp - 1};
    case Kernel_SunDepth: return GPU_String{kTokenSun, sizeof kTokenSun - 1};
    case Kernel_Geometry: return GPU_String{kTokenGeometry, sizeof kTokenGeometry - 1};
    case Kernel_Voxelize: return GPU_String{kTokenVoxelize, sizeof kTokenVoxelize - 1};
    default: return GPU_String{nullptr, 0};
    }
}

static GPU_GLSLError g_last_error;
static char g_last_error_text[512];

GPU_API GPU_String GPU_SPIRVFromGLSL(DS_Arena* arena, GPU_ShaderStage stage, GPU_PipelineLayout* layout, const GPU_ShaderDesc* desc, GPU_GLSLErrorArray* out_errors) {
    (void)arena; (void)layout;
    GPU_String empty = {nullptr, 0};
    GPU_REQUIRE(desc, empty, "GPU_SPIRVFromGLSL: NULL shader desc");
    GPU_ShaderDesc probe = *desc;
    probe.spirv = empty;
    KernelId k = identify_shader(&probe);
    bool stage_ok = (k == Kernel_Lighting || is_post_kernel(k) || k == Kernel_SunDepth || k == Kernel_Geometry || k == Kernel_Voxelize) ? (stage == GPU_ShaderStage_Vertex || stage == GPU_ShaderStage_Fragment)
                                           : (stage == GPU_ShaderStage_Compute);
    if (k != Kernel_None && stage_ok) {
        if (out_errors) { out_errors->data = nullptr; out_errors->length = 0; }
        return token_for(k);
    }
    snprintf(g_last_error_text, sizeof g_last_error_text,
             "the HIP backend has no built-in kernel for shader \"%s\" (stage %d); supported: gen_brdf_integration_map.glsl, "
             "gen_irradiance_map.glsl, gen_prefiltered_env_map.glsl, lightgrid_sweep.glsl (compute), lighting_pass.glsl, taa_resolve.glsl, bloom_downsample.glsl, bloom_upsample.glsl, final_post_process.glsl (full-screen), sun_depth_pass.glsl (depth-only raster), geometry_pass.glsl (G-buffer raster), lightgrid_voxelize.glsl (conservative raster into the light grid)",
             basename_of(desc->glsl_debug_filepath).c_str(), (int)stage);
    if (!out_errors) { gpu_fail("GPU_SPIRVFromGLSL: %s", g_last_error_text); return empty; }
    g_last_error.shader_stage = stage; g_last_error.line = 0;
    g_last_error.error_message = GPU_String{g_last_error_text, strlen(g_last_error_text)};
    out_errors->data = &g_last_error; out_errors->length = 1;
    return empty;
}

GPU_API GPU_String GPU_JoinGLSLErrorString(DS_Arena* arena, GPU_GLSLErrorArray errors) {
    (void)arena;
    static std::string joined;
    joined.clear();
    for (uint32_t i = 0; i < errors.length; ++i) {
        char head[64];
        snprintf(head, sizeof head, "line %u: ", errors.data[i].line);
        joined += head;
        joined.append(errors.data[i].error_message.data, errors.data[i].error_message.length);
        joined += "\n";
    }
    return GPU_String{joined.c_str(), joined.size()};
}

GPU_API GPU_ComputePipeline* GPU_MakeComputePipeline(GPU_PipelineLayout* layout, const GPU_ShaderDesc* cs) {
    GPU_REQUIRE(layout && layout->finalized && cs, nullptr, "GPU_MakeComputePipeline: NULL / unfinalised argument");
    KernelId k = identify_shader(cs);
    GPU_REQUIRE(k == Kernel_BrdfLut || k == Kernel_Irradiance || k == Kernel_Prefilter || k == Kernel_LightgridSweep, nullptr,
                "GPU_MakeComputePipeline: shader \"%s\" has no built-in HIP kernel", basename_of(cs->glsl_debug_filepath).c_str());
    if (k == Kernel_LightgridSweep) {                                          // lightgrid_sweep.glsl:3 GPU_BINDING(IMG0) image3D
        int b = find_binding(layout, "IMG0");
        GPU_REQUIRE(b >= 0 && layout->bindings[b].kind == Bind_StorageImage, nullptr, "GPU_MakeComputePipeline: layout has no \"IMG0\" storage image");
        GPU_ComputePipeline* p = new GPU_ComputePipeline();
        p->layout = layout; p->kernel = k;
        return p;
    }
    GPU_REQUIRE(find_binding(layout, "OUTPUT") >= 0, nullptr, "GPU_MakeComputePipeline: layout has no \"OUTPUT\" storage image");
    if (k != Kernel_BrdfLut)
        GPU_REQUIRE(find_binding(layout, "TEX_ENV_CUBE") >= 0, nullptr, "GPU_MakeComputePipeline: layout has no \"TEX_ENV_CUBE\" texture");
    GPU_ComputePipeline* p = new GPU_ComputePipeline();
    p->layout = layout; p->kernel = k;
    return p;
}
GPU_API void GPU_DestroyComputePipeline(GPU_ComputePipeline* p) { delete p; }

GPU_API GPU_RenderPass* GPU_MakeRenderPass(const GPU_RenderPassDesc* desc) {
    GPU_REQUIRE(desc, nullptr, "GPU_MakeRenderPass: NULL desc");
    GPU_REQUIRE(desc->color_targets != GPU_SWAPCHAIN_COLOR_TARGET, nullptr, "GPU_MakeRenderPass: swapchain targets are unsupported (headless backend)");
    GPU_REQUIRE(desc->msaa_color_resolve_targets == nullptr, nullptr, "GPU_MakeRenderPass: MSAA is unsupported (raster)");
    GPU_RenderPass* rp = new GPU_RenderPass();
    rp->desc = *desc;
    for (uint32_t i = 0; i < desc->color_targets_count; ++i) rp->targets.push_back(desc->color_targets[i]);
    rp->desc.color_targets = rp->targets.data();
    if ((rp->desc.width == 0 || rp->desc.height == 0) && !rp->targets.empty() && rp->targets[0].texture) {   // size left to the target (the swapchain pass, render.cpp:782-785)
        rp->desc.width = mip_dim(rp->targets[0].texture->width, rp->targets[0].mip_level);
        rp->desc.height = mip_dim(rp->targets[0].texture->height, rp->targets[0].mip_level);
    }
    if ((rp->desc.width == 0 || rp->desc.height == 0) && rp->targets.empty() && desc->depth_stencil_target) {   // depth-only pass (render.cpp:725-729)
        rp->desc.width = desc->depth_stencil_target->width;
        rp->desc.height = desc->depth_stencil_target->height;
    }
    return rp;
}
GPU_API void GPU_DestroyRenderPass(GPU_RenderPass* rp) { delete rp; }

static hipEvent_t next_event(GPU_Graph* g, size_t& used) {
    if (used == g->ev.size()) { hipEvent_t e; HIP_OK(hipEventCreate(&e)); g->ev.push_back(e); }
    return g->ev[used++];
}

// Runs `launch` bracketed by events when timing is on.
template <class F>
static void timed(GPU_Graph* g, const std::string& name, size_t& ev_used, F launch) {
    if (G.timing) {
        hipEvent_t a = next_event(g, ev_used);
        HIP_OK(hipEventRecord(a, g->cur));
        launch();
        hipEvent_t b = next_event(g, ev_used);
        HIP_OK(hipEventRecord(b, g->cur));
        g->timed_names.push_back(name);
    } else {
        launch();
    }
}

// Globals as they are at submit time: the caller fills the persistently mapped buffer before GPU_GraphSubmit (render.cpp:991)
static void read_globals(const BufferImpl* buf, size_t offset, void* dst, size_t bytes) {
    if (buf->pinned_host) memcpy(dst, (const char*)buf->dev + offset, bytes);
    else HIP_OK(hipMemcpy(dst, (const char*)buf->dev + offset, bytes, hipMemcpyDeviceToHost));
}

// ------------------------------------------------------------------------------------------
// raster jobs: sun depth (K12, render.cpp:993-1020), geometry (K13, :1076-1115), voxelise (K14, :1039-1056)
// ------------------------------------------------------------------------------------------
// The draws of one render-pass instance are ONE raster job (one Op_Raster): merging them is exact (K12: a per-pixel minimum; K13:
// depth, then triangle number; K14: which store to a voxel wins follows the triangles' submission order, which merging keeps:
// DESIGN.md K14), and one setup + one tile launch replace hundreds of per-part launches.  A job is closed (its scratch sized from the
// known triangle count, no read-back) at GPU_OpEndRenderPass, or when its kind's same_job says that a draw cannot go on in it.
// A kind's row holds what the jobs differ in on the host; the shared code at the end of the section reads it from the pipeline.
struct RasterKind {
    const char* op_name; const char* tag; const char* stage[2];              // stage: what GPUX_GraphTimedOpName calls the two launches
    const char* shader; const char* pass_name; GPU_CullMode cull; const char* cull_name;
    bool indexed;                                                             // drawn by GPU_OpDrawIndexed (false: by GPU_OpDraw)
    size_t globals_bytes; const char* globals_msg;                            // what the kind reads of GLOBALS, and the refusal of a smaller buffer
    size_t draw_bytes; size_t (*scratch_bytes)(uint32_t, int, int);
    bool (*pipeline_ok)(const RasterKind& rk, const GPU_GraphicsPipelineDesc* desc);      // refuses every state the kind is not implemented for
    // one draw: checks the bindings of d.set that the kind reads and the range of `count` indices from d.first_index, in the order the
    // kind has always had; fills in the draw's buffers (d.vb, d.ib) and target
    bool (*draw_ok)(GPU_Graph* g, uint32_t count, const char* fn, RasterDraw& d);
    // does the draw go on in the open job of its pass?  (false: that job is closed and the draw opens the next one)
    bool (*same_job)(const Op& job, const GPU_GraphicsPipeline* pipe, const RasterDraw& d);
    bool (*fill_draw)(const RasterDraw& d, void* out);                       // the draw's entry of the job's draw table, at submit
    int (*launch)(const Op& op, const RasterScratch& rs, hipStream_t st, int stage);      // fills the kind's Pbrk*Args, launches stage 0 or 1
};

// What K12 and K13 ask, in the order the checks have always had (K13 checks its colour targets between the two): the pass covers its
// whole depth target (a texture has no zero extent, so width > 0 adds nothing to K12); depth test and write, the pass's cull mode,
// nothing blended.
static bool raster_target_ok(const GPU_GraphicsPipelineDesc* desc, const RasterKind& rk) {
    const GPU_RenderPassDesc& rd = desc->render_pass->desc;
    const GPU_Texture* dt = rd.depth_stencil_target;
    GPU_REQUIRE(rd.width > 0 && rd.height > 0 && rd.width <= 16384 && rd.height <= 16384 && dt->width == rd.width && dt->height == rd.height && dt->layer_count == 1 && dt->depth == 1, false,
                "GPU_MakeGraphicsPipeline: the %s pass must cover its whole 2-D depth target (at most 16384^2)", rk.pass_name);
    return true;
}
static bool raster_state_ok(const GPU_GraphicsPipelineDesc* desc, const RasterKind& rk) {
    GPU_REQUIRE(desc->enable_depth_test && desc->enable_depth_write, false, "GPU_MakeGraphicsPipeline: %s is implemented with depth test + depth write only", rk.shader);
    GPU_REQUIRE(desc->cull_mode == rk.cull, false, "GPU_MakeGraphicsPipeline: %s is implemented for %s", rk.shader, rk.cull_name);
    GPU_REQUIRE(!desc->enable_blending && !desc->enable_conservative_rasterization, false,
                "GPU_MakeGraphicsPipeline: blending and conservative rasterisation are not implemented for %s", rk.shader);
    return true;
}
// K12: depth test + write, two-sided, position first; anything else would need a raster feature this backend does not have
static bool sun_pipeline_ok(const RasterKind& rk, const GPU_GraphicsPipelineDesc* desc) {
    const GPU_RenderPassDesc& rd = desc->render_pass->desc;
    const GPU_Texture* dt = rd.depth_stencil_target;
    GPU_REQUIRE(dt && dt->format == GPU_Format_D32F_Or_X8D24UN && rd.color_targets_count == 0, false,
                "GPU_MakeGraphicsPipeline: sun_depth_pass.glsl needs a render pass with a D32F depth target and no colour targets (render.cpp:725-729)");
    if (!raster_target_ok(desc, rk) || !raster_state_ok(desc, rk)) return false;
    GPU_REQUIRE(desc->vertex_input_formats && desc->vertex_input_formats_count > 0 && desc->vertex_input_formats[0] == GPU_Format_RGB32F, false,
                "GPU_MakeGraphicsPipeline: sun_depth_pass.glsl reads an RGB32F position as its first vertex attribute");
    return true;
}
// K13: exactly the reference's state (render.cpp:190-233, 700-708)
static bool geo_pipeline_ok(const RasterKind& rk, const GPU_GraphicsPipelineDesc* desc) {
    const GPU_RenderPassDesc& rd = desc->render_pass->desc;
    const GPU_Texture* dt = rd.depth_stencil_target;
    GPU_REQUIRE(rd.color_targets_count == 5 && dt && dt->format == GPU_Format_D32F_Or_X8D24UN, false,
                "GPU_MakeGraphicsPipeline: geometry_pass.glsl needs a render pass with five colour targets and a D32F depth target (render.cpp:700-708)");
    if (!raster_target_ok(desc, rk)) return false;
    for (uint32_t i = 0; i < 5; ++i) {
        const GPU_Texture* ct = desc->render_pass->targets[i].texture;
        GPU_REQUIRE(ct && desc->render_pass->targets[i].mip_level == 0 && ct->format == (i < 4 ? GPU_Format_RGBA8UN : GPU_Format_RG16F) &&
                    ct->width == rd.width && ct->height == rd.height && ct->layer_count == 1 && ct->depth == 1, false,
                    "GPU_MakeGraphicsPipeline: geometry pass colour target %u must be a %ux%u 2D %s texture (render.cpp:680-691)", i, rd.width, rd.height, i < 4 ? "RGBA8UN" : "RG16F");
    }
    if (!raster_state_ok(desc, rk)) return false;
    GPU_REQUIRE(desc->vertex_input_formats && desc->vertex_input_formats_count == 4 && desc->vertex_input_formats[0] == GPU_Format_RGB32F &&
                desc->vertex_input_formats[1] == GPU_Format_RGB32F && desc->vertex_input_formats[2] == GPU_Format_RGB32F && desc->vertex_input_formats[3] == GPU_Format_RG32F, false,
                "GPU_MakeGraphicsPipeline: geometry_pass.glsl reads the 44-byte Vertex (RGB32F x3, RG32F; render.cpp:227)");
    for (const char* name : {"GLOBALS", "TEX0", "TEX1", "TEX_ORM", "TEX_EMISSIVE", "SAMPLER_LINEAR_WRAP"})
        GPU_REQUIRE(find_binding(desc->layout, name) >= 0, false, "GPU_MakeGraphicsPipeline: the geometry pass layout has no \"%s\" binding", name);
    return true;
}
// K14: exactly the reference's state (render.cpp:113-149, 711-714): a pass without targets, no vertex inputs, conservative
static bool vox_pipeline_ok(const RasterKind& rk, const GPU_GraphicsPipelineDesc* desc) {
    const GPU_RenderPassDesc& rd = desc->render_pass->desc;
    GPU_REQUIRE(rd.color_targets_count == 0 && rd.depth_stencil_target == nullptr, false,
                "GPU_MakeGraphicsPipeline: lightgrid_voxelize.glsl needs a render pass without colour and depth targets (render.cpp:711-714)");
    GPU_REQUIRE(rd.width == rd.height && rd.width >= 8 && rd.width <= 256 && (rd.width & 7) == 0, false,
                "GPU_MakeGraphicsPipeline: the voxelise pass must be N x N with N a multiple of 8 in 8 .. 256 (got %u x %u)", rd.width, rd.height);
    GPU_REQUIRE(desc->vertex_input_formats_count == 0, false, "GPU_MakeGraphicsPipeline: lightgrid_voxelize.glsl has no vertex inputs (it reads SSBO0 / SSBO1)");
    GPU_REQUIRE(desc->enable_conservative_rasterization, false, "GPU_MakeGraphicsPipeline: lightgrid_voxelize.glsl is implemented with conservative rasterisation only (render.cpp:147)");
    GPU_REQUIRE(desc->cull_mode == rk.cull, false, "GPU_MakeGraphicsPipeline: %s is implemented for %s", rk.shader, rk.cull_name);
    GPU_REQUIRE(!desc->enable_depth_test && !desc->enable_depth_write && !desc->enable_blending, false,
                "GPU_MakeGraphicsPipeline: lightgrid_voxelize.glsl is implemented without depth test, depth write and blending");
    static const struct { const char* name; BindKind kind; } need[] = {{"GLOBALS", Bind_Buffer}, {"SSBO0", Bind_Buffer}, {"SSBO1", Bind_Buffer},
        {"IMG0", Bind_StorageImage}, {"SUN_DEPTH_MAP", Bind_Texture}, {"TEX0", Bind_Texture}, {"TEX_EMISSIVE", Bind_Texture},
        {"SAMPLER_PERCENTAGE_CLOSER", Bind_Sampler}, {"SAMPLER_LINEAR_WRAP", Bind_Sampler}};
    for (const auto& nb : need) {
        const int b = find_binding(desc->layout, nb.name);
        GPU_REQUIRE(b >= 0 && desc->layout->bindings[(size_t)b].kind == nb.kind, false, "GPU_MakeGraphicsPipeline: the voxelise pass layout has no \"%s\" binding of the right kind", nb.name);
    }
    return true;
}

static bool index_range_ok(const BufferImpl* ib, uint32_t first, uint32_t count, const char* fn, const char* msg) {
    const uint64_t n_idx = ib->base.size / 4;                                 // 32-bit indices (gpu_vulkan.c:2591-2593)
    GPU_REQUIRE((uint64_t)first + count <= n_idx, false, msg, fn, first, (unsigned long long)first + count, (unsigned long long)n_idx);
    return true;
}
// K12 and K13 read the buffers bound on the graph and write the pass's depth target; K12 reads no binding but GLOBALS
static bool sun_draw_ok(GPU_Graph* g, uint32_t count, const char* fn, RasterDraw& d) {
    GPU_REQUIRE(g->vertex_buffer, false, "%s: no vertex buffer bound (GPU_OpBindVertexBuffer)", fn);
    GPU_REQUIRE(g->index_buffer, false, "%s: no index buffer bound (GPU_OpBindIndexBuffer)", fn);
    d.vb = g->vertex_buffer; d.ib = g->index_buffer; d.target = (TextureImpl*)g->in_pass->desc.depth_stencil_target;
    return index_range_ok(d.ib, d.first_index, count, fn, "%s: indices [%u, %llu) lie outside the bound index buffer (%llu indices)");
}
static bool geo_draw_ok(GPU_Graph* g, uint32_t count, const char* fn, RasterDraw& d) {
    for (const char* name : {"TEX0", "TEX1", "TEX_ORM", "TEX_EMISSIVE"}) {
        Slot* sl = named_slot(d.set, name);
        GPU_REQUIRE(sl && sl->tex, false, "%s: geometry pass: \"%s\" is not bound", fn, name);
        GPU_REQUIRE(is_material_2d(sl->tex) && sl->whole, false,
                    "%s: geometry pass: \"%s\" must be a whole 2D RGBA8UN, BC1, BC3 or BC5 texture", fn, name);
    }
    Slot* sm = named_slot(d.set, "SAMPLER_LINEAR_WRAP");
    GPU_REQUIRE(sm && sm->sampler == &G.samplers[0], false, "%s: geometry pass: \"SAMPLER_LINEAR_WRAP\" must be GPU_SamplerLinearWrap()", fn);
    GPU_REQUIRE(g->push_size == 16, false, "%s: the geometry pass needs its 16-byte push constants (taa_jitter, taa_jitter_prev; render.cpp:1091-1094)", fn);
    return sun_draw_ok(g, count, fn, d);
}
// K14 reads SSBO0 / SSBO1 of the draw's set (from vertex d.first_index on) and stores into the set's IMG0
static bool vox_draw_ok(GPU_Graph* g, uint32_t count, const char* fn, RasterDraw& d) {
    const uint32_t N = g->in_pass->desc.width;
    Slot* vb = named_slot(d.set, "SSBO0");
    Slot* ib = named_slot(d.set, "SSBO1");
    GPU_REQUIRE(vb && vb->buf, false, "%s: voxelise pass: \"SSBO0\" (vertices) is not a bound buffer", fn);
    GPU_REQUIRE(ib && ib->buf, false, "%s: voxelise pass: \"SSBO1\" (indices) is not a bound buffer", fn);
    if (!index_range_ok(ib->buf, d.first_index, count, fn, "%s: voxelise pass: vertices [%u, %llu) lie outside \"SSBO1\" (%llu indices)")) return false;
    Slot* img = named_slot(d.set, "IMG0");
    GPU_REQUIRE(img && img->tex && img->mip == 0 && img->tex->base.format == GPU_Format_RGBA16F && img->tex->base.layer_count == 1 &&
                img->tex->base.width == N && img->tex->base.height == N && img->tex->base.depth == N, false,
                "%s: voxelise pass: \"IMG0\" must be mip 0 of a %u^3 RGBA16F 3-D storage image", fn, N);
    Slot* sun = named_slot(d.set, "SUN_DEPTH_MAP");
    GPU_REQUIRE(sun && sun->tex && sun->whole && sun->tex->base.format == GPU_Format_D32F_Or_X8D24UN && sun->tex->base.layer_count == 1 && sun->tex->base.depth == 1, false,
                "%s: voxelise pass: \"SUN_DEPTH_MAP\" must be a whole 2D D32F texture (render.cpp:676)", fn);
    for (const char* name : {"TEX0", "TEX_EMISSIVE"}) {
        Slot* sl = named_slot(d.set, name);
        GPU_REQUIRE(sl && sl->tex && sl->whole && is_material_2d(sl->tex), false,
                    "%s: voxelise pass: \"%s\" must be a whole 2D RGBA8UN, BC1, BC3 or BC5 texture", fn, name);
    }
    Slot* sm = named_slot(d.set, "SAMPLER_LINEAR_WRAP");
    GPU_REQUIRE(sm && sm->sampler == &G.samplers[0], false, "%s: voxelise pass: \"SAMPLER_LINEAR_WRAP\" must be GPU_SamplerLinearWrap()", fn);
    Slot* pc = named_slot(d.set, "SAMPLER_PERCENTAGE_CLOSER");
    GPU_REQUIRE(pc && pc->sampler && pc->sampler->desc.min_filter == GPU_Filter_Linear && pc->sampler->desc.mag_filter == GPU_Filter_Linear &&
                pc->sampler->desc.address_modes[0] == GPU_AddressMode_Clamp && pc->sampler->desc.address_modes[1] == GPU_AddressMode_Clamp &&
                pc->sampler->desc.compare_op == GPU_CompareOp_Less, false,
                "%s: voxelise pass: \"SAMPLER_PERCENTAGE_CLOSER\" must be a linear / clamp / GPU_CompareOp_Less sampler (render.cpp:664-673)", fn);
    d.vb = vb->buf; d.ib = ib->buf; d.target = img->tex;
    return true;
}

// K12's draws share the job's vertex / index pair and stride; K13's name their own buffers; K14's share the job's grid
static bool sun_same_job(const Op& job, const GPU_GraphicsPipeline* pipe, const RasterDraw& d) { return job.buf == d.vb && job.buf2 == d.ib && job.gpipe->vertex_stride == pipe->vertex_stride; }
static bool geo_same_job(const Op&, const GPU_GraphicsPipeline*, const RasterDraw&) { return true; }
static bool vox_same_job(const Op& job, const GPU_GraphicsPipeline*, const RasterDraw& d) { return job.tex == d.target; }

// The draw tables of the raster jobs, filled from what every draw's GLOBALS holds now (the caller fills the mapped Globals before
// submitting, render.cpp:991), before anything is launched.
static bool fill_sun_draw(const RasterDraw& d, void* out) {
    PbrkRasterDraw& o = *(PbrkRasterDraw*)out;
    read_globals(named_slot(d.set, "GLOBALS")->buf, 384, o.m, 64);           // render.h:129: sun_space_from_world
    // an orthographic matrix (last row (0, 0, 0, c > 0)) needs no near-plane clip
    GPU_REQUIRE(o.m[3] == 0.0f && o.m[7] == 0.0f && o.m[11] == 0.0f && o.m[15] > 0.0f, false,
                "GPU_GraphSubmit: perspective sun projection not implemented (sun_space_from_world's last row must be (0, 0, 0, c > 0))");
    o.first_tri = d.first_tri; o.first_index = d.first_index; o.vertex_offset = d.vertex_offset; o.pad = 0;
    return true;
}
static PbrkGeoTex material_tex(const TextureImpl* t) { return {material_texels(t), (int)t->base.width, (int)t->base.height, (int)t->base.mip_level_count, 0}; }
// the post passes' view of a whole 2-D texture, and the PBRK_FMT_* of the colour target they store to
static PbrkTex2D tex2d(const TextureImpl* t, int fmt) { PbrkTex2D r; r.data = t->dev; r.format = fmt; r.width = (int)t->base.width; r.height = (int)t->base.height; return r; }
static int out_fmt(GPU_Format f) {
    return f == GPU_Format_RGBA16F ? PBRK_FMT_RGBA16F : (f == GPU_Format_RGBA32F ? PBRK_FMT_RGBA32F : (f == GPU_Format_RGBA8UN ? PBRK_FMT_RGBA8UN : PBRK_FMT_BGRA8UN));
}
static bool fill_geo_draw(const RasterDraw& d, void* out) {               // both matrices, the draw's textures and buffers
    PbrkGeoDraw& o = *(PbrkGeoDraw*)out;
    memset(&o, 0, sizeof o);
    const BufferImpl* gb = named_slot(d.set, "GLOBALS")->buf;
    read_globals(gb, 0, o.m, 64); read_globals(gb, 448, o.m_old, 64);      // render.h:123, :130
    memcpy(o.jitter, d.push, 8); memcpy(o.jitter_prev, d.push + 2, 8);
    static const char* const names[4] = {"TEX0", "TEX1", "TEX_ORM", "TEX_EMISSIVE"};
    for (int k = 0; k < 4; ++k) o.tex[k] = material_tex(named_slot(d.set, names[k])->tex);
    o.vertices = d.vb->dev; o.indices = (const uint32_t*)d.ib->dev; o.vertex_count = d.vb->base.size / 44u;
    o.first_tri = d.first_tri; o.first_index = d.first_index; o.vertex_offset = d.vertex_offset;
    return true;
}
static bool fill_vox_draw(const RasterDraw& d, void* out) {               // sun matrix and direction, scale, the draw's buffers and textures
    PbrkVoxDraw& o = *(PbrkVoxDraw*)out;
    memset(&o, 0, sizeof o);
    const BufferImpl* gb = named_slot(d.set, "GLOBALS")->buf;
    read_globals(gb, 384, o.sun, 64); read_globals(gb, 512, o.sun_dir, 16); read_globals(gb, 544, &o.scale, 4);    // render.h:129, :131, :134
    o.first_tri = d.first_tri; o.first_vertex = d.first_index;
    o.vertices = (const float*)d.vb->dev; o.vertex_floats = d.vb->base.size / 4u; o.indices = (const uint32_t*)d.ib->dev;
    const TextureImpl* sun = named_slot(d.set, "SUN_DEPTH_MAP")->tex;
    o.sun_depth = (const float*)sun->dev; o.sun_w = (int)sun->base.width; o.sun_h = (int)sun->base.height;
    static const char* const names[2] = {"TEX0", "TEX_EMISSIVE"};
    for (int k = 0; k < 2; ++k) o.tex[k] = material_tex(named_slot(d.set, names[k])->tex);
    return true;
}

static int sun_launch(const Op& op, const RasterScratch& rs, hipStream_t st, int stage) {
    PbrkRasterArgs a;
    a.vertices = op.buf->dev; a.vertex_stride = op.gpipe->vertex_stride; a.vertex_count = op.buf->base.size / a.vertex_stride; a.indices = (const uint32_t*)op.buf2->dev;
    a.draws = (const PbrkRasterDraw*)rs.draws_dev; a.draw_count = (uint32_t)op.draws.size(); a.tri_count = op.tri_count;
    a.depth = (float*)op.tex->dev; a.width = (int)op.tex->base.width; a.height = (int)op.tex->base.height;
    a.scratch = rs.dev; a.rejected = G.raster_rejected;
    return stage == 0 ? pbrk_raster_setup(&a, st) : pbrk_raster_tiles(&a, st);
}
static int geo_launch(const Op& op, const RasterScratch& rs, hipStream_t st, int stage) {
    PbrkGeometryArgs a;
    a.draws = (const PbrkGeoDraw*)rs.draws_dev; a.draw_count = (uint32_t)op.draws.size(); a.tri_count = op.tri_count;
    for (int k = 0; k < 4; ++k) a.color[k] = ((TextureImpl*)op.pass->targets[(size_t)k].texture)->dev;
    a.velocity = ((TextureImpl*)op.pass->targets[4].texture)->dev;
    a.depth = (float*)op.tex->dev; a.width = (int)op.tex->base.width; a.height = (int)op.tex->base.height;
    a.scratch = rs.dev; a.rejected = G.raster_rejected;
    return stage == 0 ? pbrk_geometry_setup(&a, st) : pbrk_geometry_tiles(&a, st);
}
static int vox_launch(const Op& op, const RasterScratch& rs, hipStream_t st, int stage) {
    PbrkVoxelizeArgs a;
    a.draws = (const PbrkVoxDraw*)rs.draws_dev; a.draw_count = (uint32_t)op.draws.size(); a.tri_count = op.tri_count;
    a.grid = op.tex->dev; a.n = (int)op.tex->base.width;
    a.scratch = rs.dev; a.rejected = G.raster_rejected; a.fragments = G.raster_rejected + 1;
    return stage == 0 ? pbrk_voxelize_cover(&a, st) : pbrk_voxelize_resolve(&a, st);
}

static const RasterKind kSunDepthJob = {"K12.sun_depth", "K12", {"K12.setup", "K12.tiles"}, "sun_depth_pass.glsl", "sun depth", GPU_CullMode_TwoSided, "GPU_CullMode_TwoSided only", true,
    448, "%s: \"GLOBALS\" must be a buffer that holds sun_space_from_world (render.h:122-136)", sizeof(PbrkRasterDraw), pbrk_raster_scratch_bytes, sun_pipeline_ok, sun_draw_ok, sun_same_job, fill_sun_draw, sun_launch};
static const RasterKind kGeometryJob = {"K13.geometry", "K13", {"K13.setup", "K13.tiles"}, "geometry_pass.glsl", "geometry", GPU_CullMode_DrawCCW, "GPU_CullMode_DrawCCW only (render.cpp:232)", true,
    512, "%s: \"GLOBALS\" must be a buffer that holds old_clip_space_from_world (render.h:122-136)", sizeof(PbrkGeoDraw), pbrk_geometry_scratch_bytes, geo_pipeline_ok, geo_draw_ok, geo_same_job, fill_geo_draw, geo_launch};
static const RasterKind kVoxelizeJob = {"K14.voxelize", "K14", {"K14.cover", "K14.resolve"}, "lightgrid_voxelize.glsl", "voxelise", GPU_CullMode_TwoSided, "GPU_CullMode_TwoSided only", false,
    548, "%s: voxelise pass: \"GLOBALS\" must be a buffer that holds lightgrid_scale (548 bytes, render.h:122-136)", sizeof(PbrkVoxDraw), pbrk_voxelize_scratch_bytes, vox_pipeline_ok, vox_draw_ok, vox_same_job, fill_vox_draw, vox_launch};

// ---- the shared path: record, close, snapshot, execute ----
static const RasterKind* bound_raster_row(const GPU_Graph* g) { return g->in_pass && g->bound_draw >= 0 ? g->draw_params[(size_t)g->bound_draw].pipeline->raster : nullptr; }

static void close_raster_job(GPU_Graph* g) {
    if (g->raster_op < 0) return;
    Op& op = g->ops[(size_t)g->raster_op];
    g->raster_op = -1;
    if ((size_t)op.raster_slot >= g->raster.size()) g->raster.resize((size_t)op.raster_slot + 1);
    RasterScratch& rs = g->raster[(size_t)op.raster_slot];
    const RasterKind& rk = *op.gpipe->raster;
    const size_t need = rk.scratch_bytes(op.tri_count, (int)op.tex->base.width, (int)op.tex->base.height);
    bool ok = true;
    if (rs.dev_bytes < need) {
        (void)hipFree(rs.dev); rs.dev = nullptr; rs.dev_bytes = 0;
        if (hipMalloc(&rs.dev, need) == hipSuccess) rs.dev_bytes = need; else { rs.dev = nullptr; ok = false; }
    }
    const size_t table = op.draws.size() * rk.draw_bytes;
    if (ok && rs.draws_cap < table) {
        (void)hipFree(rs.draws_dev); (void)hipHostFree(rs.draws_host); rs.draws_dev = nullptr; rs.draws_host = nullptr; rs.draws_cap = 0;
        if (hipMalloc(&rs.draws_dev, table) == hipSuccess && hipHostMalloc((void**)&rs.draws_host, table, hipHostMallocDefault) == hipSuccess) rs.draws_cap = table;
        else ok = false;
    }
    if (ok && !G.raster_rejected) {
        if (hipMalloc((void**)&G.raster_rejected, 16) != hipSuccess || hipMemset(G.raster_rejected, 0, 16) != hipSuccess) { G.raster_rejected = nullptr; ok = false; }
    }
    if (!ok) { (void)hipGetLastError(); op.tri_count = 0; op.draws.clear(); gpu_fail("GPU_OpEndRenderPass: allocation of the raster scratch (%zu bytes) failed", need); }
}

// One draw of a raster job (fn: the entry point).  Everything a launch could trip over is checked here.
static void record_raster_draw(GPU_Graph* g, const DrawParams& dp, uint32_t count, uint32_t instance_count, uint32_t first, uint32_t vertex_offset, const char* fn) {
    const RasterKind& rk = *dp.pipeline->raster;
    GPU_REQUIRE_V(dp.pipeline->pass == g->in_pass, "%s: pipeline was created for a different render pass", fn);
    GPU_REQUIRE_V(dp.set->layout == dp.pipeline->layout, "%s: descriptor set and pipeline use different layouts", fn);
    Slot* gl = named_slot(dp.set, "GLOBALS");
    GPU_REQUIRE_V(gl && gl->buf && gl->buf->base.size >= rk.globals_bytes, rk.globals_msg, fn);
    RasterDraw d; d.set = dp.set; d.first_index = first; d.vertex_offset = vertex_offset; memcpy(d.push, g->push, sizeof d.push);
    if (!rk.draw_ok(g, count, fn, d)) return;
    const uint32_t tris = count / 3;                                          // whole triangles only
    if (tris == 0 || instance_count == 0) return;                             // any instance count > 0 draws the same triangles once
    if (g->raster_op >= 0) {
        const Op& cur = g->ops[(size_t)g->raster_op];
        GPU_REQUIRE_V(cur.gpipe->raster == &rk, "%s: a %s draw inside another raster pass", fn, rk.pass_name);
        if (!rk.same_job(cur, dp.pipeline, d)) close_raster_job(g);
    }
    if (g->raster_op < 0) {
        Op op; op.kind = Op_Raster; op.name = rk.op_name;
        op.pass = g->in_pass; op.gpipe = dp.pipeline; op.tex = d.target; op.buf = d.vb; op.buf2 = d.ib;
        op.raster_slot = (int)g->raster_used++;
        g->ops.push_back(op);
        g->raster_op = (int)g->ops.size() - 1;
    }
    Op& op = g->ops[(size_t)g->raster_op];
    GPU_REQUIRE_V((uint64_t)op.tri_count + tris <= (1u << 26), "%s: more than 2^26 triangles in one %s pass", fn, rk.pass_name);
    d.first_tri = op.tri_count;
    op.draws.push_back(d);
    op.tri_count += tris;
}

static bool snapshot_raster_draws(GPU_Graph* g) {
    for (const Op& op : g->ops) {
        if (op.kind != Op_Raster || !op.tri_count) continue;
        const RasterKind& rk = *op.gpipe->raster;
        char* table = (char*)g->raster[(size_t)op.raster_slot].draws_host;
        for (size_t i = 0; i < op.draws.size(); ++i) if (!rk.fill_draw(op.draws[i], table + i * rk.draw_bytes)) return false;
    }
    return true;
}

// A raster job: upload the draw table that GPU_GraphSubmit snapshotted, then its two launches
static void exec_raster(GPU_Graph* g, Op& op, size_t& ev_used) {
    if (!op.tri_count) return;
    RasterScratch& rs = g->raster[(size_t)op.raster_slot];
    const RasterKind& rk = *op.gpipe->raster;
    for (int stage = 0; stage < 2; ++stage)
        timed(g, rk.stage[stage], ev_used, [&] {
            if (stage == 0) HIP_OK(hipMemcpyAsync(rs.draws_dev, rs.draws_host, op.draws.size() * rk.draw_bytes, hipMemcpyHostToDevice, g->cur));
            int rc = rk.launch(op, rs, g->cur, stage);
            if (rc != PBRK_OK) gpu_fail("%s %s launch failed (%d)", rk.tag, stage == 0 ? "setup" : "tile", rc);
        });
}

GPU_API GPU_GraphicsPipeline* GPU_MakeGraphicsPipeline(const GPU_GraphicsPipelineDesc* desc) {
    GPU_REQUIRE(desc && desc->layout && desc->render_pass, nullptr, "GPU_MakeGraphicsPipeline: NULL argument");
    KernelId k = identify_shader(&desc->fs);
    if (k == Kernel_None && identify_shader(&desc->vs) == Kernel_SunDepth) k = Kernel_SunDepth;      // the pass has a vertex stage only
    const RasterKind* rk = k == Kernel_SunDepth ? &kSunDepthJob : k == Kernel_Geometry ? &kGeometryJob : k == Kernel_Voxelize ? &kVoxelizeJob : nullptr;
    if (rk) {
        if (!rk->pipeline_ok(*rk, desc)) return nullptr;
        uint32_t stride = 0;                                  // K12: anything behind the position; K13: the 44-byte Vertex; K14: none
        for (uint32_t i = 0; i < desc->vertex_input_formats_count; ++i) {   // gpu_vulkan.c:1745-1762
            GPU_FormatInfo fi = GPUX_GetFormatInfo(desc->vertex_input_formats[i]);
            GPU_REQUIRE(fi.vertex_input, nullptr, "GPU_MakeGraphicsPipeline: vertex attribute %u has a format that is not a vertex input", i);
            stride += fi.block_size;
        }
        GPU_REQUIRE((stride & 3) == 0, nullptr, "GPU_MakeGraphicsPipeline: vertex stride %u is not a multiple of 4 bytes", stride);
        GPU_GraphicsPipeline* p = new GPU_GraphicsPipeline();
        p->layout = desc->layout; p->pass = desc->render_pass; p->kernel = k; p->shade_flags = 0; p->vertex_stride = stride; p->raster = rk;
        return p;
    }
    GPU_REQUIRE(k == Kernel_Lighting || is_post_kernel(k), nullptr,
                "GPU_MakeGraphicsPipeline: unsupported (raster): only the full-screen lighting_pass / taa_resolve / final_post_process pipelines have HIP kernels (got \"%s\")",
                basename_of(desc->fs.glsl_debug_filepath).c_str());
    GPU_REQUIRE(desc->vertex_input_formats_count == 0, nullptr, "GPU_MakeGraphicsPipeline: unsupported (raster): vertex inputs");
    GPU_REQUIRE(desc->render_pass->desc.color_targets_count == 1, nullptr, "GPU_MakeGraphicsPipeline: full-screen passes have exactly one colour target");
    GPU_GraphicsPipeline* p = new GPU_GraphicsPipeline();
    p->layout = desc->layout; p->pass = desc->render_pass; p->kernel = k; p->shade_flags = GPUX_Shade_IBL;
    if (desc->enable_blending) {                                              // gpu_vulkan.c:1828-1842
        if (!(desc->blending_mode_additive && is_bloom_kernel(k))) {
            gpu_fail("GPU_MakeGraphicsPipeline: blending is implemented for the additive bloom passes only"); delete p; return nullptr;
        }
        p->blend_additive = true;
    }
    return p;
}
GPU_API void GPU_DestroyGraphicsPipeline(GPU_GraphicsPipeline* p) { delete p; }
GPU_API void GPUX_SetShadeFlags(GPU_GraphicsPipeline* p, int flags) {
    GPU_REQUIRE_V(p, "GPUX_SetShadeFlags: NULL pipeline");
    p->shade_flags = flags;
}
GPU_API int GPUX_GetShadeFlags(GPU_GraphicsPipeline* p) {
    GPU_REQUIRE(p, 0, "GPUX_GetShadeFlags: NULL pipeline");
    return p->shade_flags;
}
GPU_API void GPUX_SetShadeSH9(GPU_GraphicsPipeline* p, GPU_Buffer* coef, uint32_t offset) {
    GPU_REQUIRE_V(p, "GPUX_SetShadeSH9: NULL pipeline");
    p->sh9_buf = (BufferImpl*)coef; p->sh9_offset = coef ? offset : 0;
}

// ------------------------------------------------------------------------------------------
// host tables -> device (cached)
// ------------------------------------------------------------------------------------------
static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static DeviceTable* get_table(int kind, int n, float roughness, int aux) {
    TableKey key = {kind, n, aux, fbits(roughness)};
    auto it = G.tables.find(key);
    if (it != G.tables.end()) return &it->second;
    DeviceTable t;
    std::vector<float> host;
    if (kind == 0) {            // prefilter (lx,ly,lz,w)
        host.resize((size_t)n * 4);
        t.count = pbrk_host_prefilter_table(n, roughness, host.data(), &t.alpha);
        t.weights.resize((size_t)(t.count > 0 ? t.count : 0));
        for (int i = 0; i < t.count; ++i) t.weights[(size_t)i] = host[(size_t)i * 4 + 3];
    } else if (kind == 1) {     // irradiance
        host.resize((size_t)n * 4);
        t.count = pbrk_host_irradiance_table(n, host.data());
    } else if (kind == 2) {     // LUT sample angles
        host.resize((size_t)n * 4);
        pbrk_host_sample_angles(n, host.data());
        t.count = n;
    } else {                    // LUT per-column view angle: V = Rotate(N, X, acos(NdotV)), gen_brdf_integration_map.glsl:154-160
        host.resize((size_t)n * 2);
        for (int x = 0; x < n; ++x) {
            float ndv = ((float)x + 0.5f) / (float)n;
            float th = acosf(ndv);
            host[2 * x] = cosf(th); host[2 * x + 1] = sinf(th);
        }
        t.count = n;
    }
    size_t bytes = host.size() * sizeof(float);
    if (bytes < 16) bytes = 16;
    hipError_t e = hipMalloc(&t.dev, bytes);
    if (e != hipSuccess) { gpu_fail("table allocation failed: %s", hipGetErrorString(e)); return nullptr; }
    HIP_OK(hipMemcpy(t.dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    // written once, never again: the Monte-Carlo kernels may keep what they derive from it (the bin cache, k_mc_region.hip 2m)
    if (kind <= 1 && t.count > 0) (void)pbrk_mc_table_register(t.dev, t.count);
    auto ins = G.tables.insert({key, t});
    return &ins.first->second;
}

// ------------------------------------------------------------------------------------------
// graphs
// ------------------------------------------------------------------------------------------
GPU_API GPU_Graph* GPU_MakeGraph(void) {
    GPU_REQUIRE(G.init, nullptr, "GPU_MakeGraph: GPU_Init has not been called");
    GPU_Graph* g = new GPU_Graph();
    HIP_OK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    return g;
}
GPU_API void GPU_MakeSwapchainGraphs(uint32_t count, GPU_Graph** out) {
    for (uint32_t i = 0; i < count; ++i) out[i] = GPU_MakeGraph();
}
GPU_API GPU_Texture* GPU_GetBackbuffer(GPU_Graph* g) { (void)g; return nullptr; }
GPU_API void* GPUX_GraphStream(GPU_Graph* g) { return g ? (void*)g->stream : nullptr; }

static void reset_graph(GPU_Graph* g) {
    g->ops.clear();
    g->submitted = false;
    g->bound_cpipe = nullptr; g->bound_cset = nullptr; g->push_size = 0;
    g->preparing = nullptr; g->in_pass = nullptr; g->draw_params.clear(); g->bound_draw = -1;
    g->vertex_buffer = nullptr; g->index_buffer = nullptr; g->raster_op = -1; g->raster_used = 0;
    g->pano_used = 0;
}
GPU_API void GPU_DestroyGraph(GPU_Graph* g) {
    GPU_REQUIRE_V(g, "GPU_DestroyGraph: NULL graph");            // the reference does not accept NULL here (gpu_vulkan.c:2393-2404)
    (void)hipStreamSynchronize(g->stream);
    for (hipStream_t s : g->side) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (hipEvent_t e : g->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->sync_ev) (void)hipEventDestroy(e);
    if (g->order_ev) (void)hipEventDestroy(g->order_ev);
    if (g->mid_ev) (void)hipEventDestroy(g->mid_ev);
    if (g->span_a) (void)hipEventDestroy(g->span_a);
    if (g->span_b) (void)hipEventDestroy(g->span_b);
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    for (RasterScratch& r : g->raster) { (void)hipFree(r.dev); (void)hipFree(r.draws_dev); (void)hipHostFree(r.draws_host); }
    (void)hipFree(g->sh_scratch);
    for (GPU_Graph::PanoTable& t : g->pano) (void)hipFree(t.dev);
    if (G.last_submitted == g) G.last_submitted = nullptr;        // idle by contract (gpu.h:453): nothing left to order against
    (void)hipStreamDestroy(g->stream);
    delete g;
}

#define REC_GUARD(g) GPU_REQUIRE_V((g) && !(g)->submitted, "%s: graph is NULL or already submitted (call GPU_GraphWait first)", __func__)

GPU_API void GPU_OpBindComputePipeline(GPU_Graph* g, GPU_ComputePipeline* p) { REC_GUARD(g); g->bound_cpipe = p; }
GPU_API void GPU_OpBindComputeDescriptorSet(GPU_Graph* g, GPU_DescriptorSet* s) {
    REC_GUARD(g);
    GPU_REQUIRE_V(s && s->finalized, "GPU_OpBindComputeDescriptorSet: set is NULL or not finalised");
    g->bound_cset = s;
}
static void push_constants(GPU_Graph* g, void* data, uint32_t size, const char* fn) {
    GPU_REQUIRE_V(g && !g->submitted, "%s: graph is NULL or already submitted", fn);
    GPU_REQUIRE_V(size <= 128 && (data || size == 0), "%s: at most 128 bytes of push constants (gpu_vulkan.c:710)", fn);
    memcpy(g->push, data, size);
    g->push_size = size;
}
GPU_API void GPU_OpPushComputeConstants(GPU_Graph* g, GPU_PipelineLayout* l, void* data, uint32_t size) { (void)l; push_constants(g, data, size, __func__); }
GPU_API void GPU_OpPushGraphicsConstants(GPU_Graph* g, GPU_PipelineLayout* l, void* data, uint32_t size) { (void)l; push_constants(g, data, size, __func__); }

// Validates a dispatch against the bound pipeline/set at record time, so that nothing can fault at launch.
static bool record_dispatch(GPU_Graph* g, Op& op, const char* fn) {
    GPU_REQUIRE(g->bound_cpipe, false, "%s: no compute pipeline bound", fn);
    GPU_REQUIRE(g->bound_cset, false, "%s: no compute descriptor set bound", fn);
    GPU_REQUIRE(g->bound_cset->layout == g->bound_cpipe->layout, false, "%s: descriptor set and pipeline use different layouts", fn);
    op.kind = Op_Dispatch;
    op.cpipe = g->bound_cpipe; op.set = g->bound_cset;
    memcpy(op.push, g->push, g->push_size); op.push_size = g->push_size;
    if (op.cpipe->kernel == Kernel_LightgridSweep) {
        Slot* img = named_slot(op.set, "IMG0");
        GPU_REQUIRE(img && img->tex, false, "%s: IMG0 is not bound", fn);
        const GPU_Texture* t = &img->tex->base;
        GPU_REQUIRE(t->format == GPU_Format_RGBA16F && t->layer_count == 1 && img->mip == 0, false, "%s: IMG0 must be mip 0 of an RGBA16F 3-D image", fn);
        GPU_REQUIRE(op.push_size >= 4, false, "%s: the sweep needs its `int X_direction` push constant (lightgrid_sweep.glsl:5-7)", fn);
        return true;
    }
    Slot* out = named_slot(op.set, "OUTPUT");
    GPU_REQUIRE(out && out->tex, false, "%s: OUTPUT is not bound", fn);
    TextureImpl* ot = out->tex;
    if (op.cpipe->kernel == Kernel_BrdfLut) {
        GPU_REQUIRE(ot->base.layer_count == 1 && ot->base.width == ot->base.height, false, "%s: BRDF LUT output must be a square 2D image", fn);
        GPU_REQUIRE(ot->base.format == GPU_Format_RG16F || ot->base.format == GPU_Format_RG32F || ot->base.format == GPU_Format_RGBA32F, false,
                    "%s: BRDF LUT output format must be RG16F, RG32F or RGBA32F", fn);
    } else {
        GPU_REQUIRE(is_f4_cube(ot), false, "%s: OUTPUT must be a square RGBA32F cubemap", fn);
        Slot* env = named_slot(op.set, "TEX_ENV_CUBE");
        GPU_REQUIRE(env && env->tex && is_f4_cube(env->tex), false, "%s: TEX_ENV_CUBE must be a square RGBA32F cubemap", fn);
        GPU_REQUIRE(env->tex != ot, false, "%s: TEX_ENV_CUBE and OUTPUT alias", fn);
    }
    return true;
}

// Sweep invocations (iy, iz) in [y0,y1) x [z0,z1): checks that every voxel they touch lies inside the image
// (direction 0 -> (x, iy, iz); 1 -> (iz, x, iy); 2 -> (iy, iz, x) with x < 128; lightgrid_sweep.glsl:10-22).
// The op keeps the ranges in row0/row1 (iy) and face0/face1 (iz).
static bool record_sweep_lines(GPU_Graph* g, Op& op, uint32_t y0, uint32_t y1, uint32_t z0, uint32_t z1, const char* fn) {
    (void)g;
    const GPU_Texture* t = &named_slot(op.set, "IMG0")->tex->base;
    int32_t dir; memcpy(&dir, op.push, 4);
    if (dir < 0 || dir > 2) dir = 2;                                          // the shader's final `else` (:19)
    uint32_t line_extent = dir == 0 ? t->width : (dir == 1 ? t->height : t->depth);
    uint32_t y_extent = dir == 0 ? t->height : (dir == 1 ? t->depth : t->width);
    uint32_t z_extent = dir == 0 ? t->depth : (dir == 1 ? t->width : t->height);
    GPU_REQUIRE(y0 < y1 && z0 < z1, false, "%s: empty line range", fn);
    GPU_REQUIRE(line_extent >= PBRK_SWEEP_LEN && y1 <= y_extent && z1 <= z_extent, false,
                "%s: sweep direction %d over lines [%u,%u) x [%u,%u) leaves the %ux%ux%u image", fn, (int)dir, y0, y1, z0, z1, t->width, t->height, t->depth);
    int32_t d32 = dir; memcpy(op.push, &d32, 4);
    op.row0 = y0; op.row1 = y1; op.face0 = z0; op.face1 = z1;
    return true;
}

GPU_API void GPUX_OpDispatchLines(GPU_Graph* g, uint32_t y0, uint32_t y1, uint32_t z0, uint32_t z1) {
    REC_GUARD(g);
    GPU_REQUIRE_V(g->in_pass == nullptr, "GPUX_OpDispatchLines: inside a render pass");
    Op op;
    if (!record_dispatch(g, op, __func__)) return;
    GPU_REQUIRE_V(op.cpipe->kernel == Kernel_LightgridSweep, "GPUX_OpDispatchLines: the bound pipeline is not the light-grid sweep");
    if (!record_sweep_lines(g, op, y0, y1, z0, z1, __func__)) return;
    op.rows_explicit = true;
    g->ops.push_back(op);
}

GPU_API void GPU_OpDispatch(GPU_Graph* g, uint32_t gx, uint32_t gy, uint32_t gz) {
    REC_GUARD(g);
    GPU_REQUIRE_V(g->in_pass == nullptr, "GPU_OpDispatch: inside a render pass");
    GPU_REQUIRE_V(gx > 0 && gy > 0 && gz > 0, "GPU_OpDispatch: zero group count");
    Op op;
    if (!record_dispatch(g, op, __func__)) return;
    op.gx = gx; op.gy = gy; op.gz = gz;
    if (op.cpipe->kernel == Kernel_LightgridSweep) {
        // local size 1x8x8 (lightgrid_sweep.glsl:1); invocation x > 0 would redo line x = 0 (base_coord.x is the constant 0, :11)
        GPU_REQUIRE_V(gx == 1, "GPU_OpDispatch: the sweep is dispatched as (1, gy, gz) (render.cpp:1072)");
        if (!record_sweep_lines(g, op, 0, gy * 8, 0, gz * 8, __func__)) return;
        g->ops.push_back(op);
        return;
    }
    Slot* out = named_slot(op.set, "OUTPUT");
    uint32_t size = mip_dim(out->tex->base.width, out->mip);
    // local size is 8x8x6 (shader line 1): the kernels work on whole rows, so the x extent must cover the image
    GPU_REQUIRE_V(gx * 8 >= size, "GPU_OpDispatch: partial-width dispatch (%u groups over %u texels) is unsupported", gx, size);
    op.face0 = 0; op.face1 = out->tex->base.layer_count;
    op.row0 = 0; op.row1 = gy * 8 < size ? gy * 8 : size;
    g->ops.push_back(op);
}

GPU_API void GPUX_OpDispatchRows(GPU_Graph* g, uint32_t face0, uint32_t face1, uint32_t row0, uint32_t row1) {
    REC_GUARD(g);
    GPU_REQUIRE_V(g->in_pass == nullptr, "GPUX_OpDispatchRows: inside a render pass");
    Op op;
    if (!record_dispatch(g, op, __func__)) return;
    GPU_REQUIRE_V(op.cpipe->kernel != Kernel_LightgridSweep, "GPUX_OpDispatchRows: use GPUX_OpDispatchLines for the light-grid sweep");
    Slot* out = named_slot(op.set, "OUTPUT");
    uint32_t size = mip_dim(out->tex->base.width, out->mip);
    GPU_REQUIRE_V(face0 < face1 && face1 <= out->tex->base.layer_count && row0 < row1 && row1 <= size,
                  "GPUX_OpDispatchRows: range faces [%u,%u) rows [%u,%u) outside a %u-layer %ux%u image", face0, face1, row0, row1,
                  out->tex->base.layer_count, size, size);
    op.face0 = face0; op.face1 = face1; op.row0 = row0; op.row1 = row1; op.rows_explicit = true;
    g->ops.push_back(op);
}

// ---- render-pass vocabulary (lighting pass only) ----
GPU_API void GPU_OpPrepareRenderPass(GPU_Graph* g, GPU_RenderPass* rp) {
    REC_GUARD(g);
    GPU_REQUIRE_V(rp && g->preparing == nullptr && g->in_pass == nullptr, "GPU_OpPrepareRenderPass: bad state");   // gpu_vulkan.c:2957
    g->preparing = rp;
    g->draw_params.clear();
}
GPU_API uint32_t GPU_OpPrepareDrawParams(GPU_Graph* g, GPU_GraphicsPipeline* p, GPU_DescriptorSet* s) {
    GPU_REQUIRE(g && g->preparing, 0, "GPU_OpPrepareDrawParams: no render pass is being prepared");              // :2964
    GPU_REQUIRE(p && s && s->finalized, 0, "GPU_OpPrepareDrawParams: NULL pipeline / unfinalised set");
    g->draw_params.push_back({p, s});
    return (uint32_t)g->draw_params.size() - 1;
}
GPU_API void GPU_OpBeginRenderPass(GPU_Graph* g) {
    REC_GUARD(g);
    GPU_REQUIRE_V(g->preparing, "GPU_OpBeginRenderPass: GPU_OpPrepareRenderPass was not called");
    g->in_pass = g->preparing; g->preparing = nullptr; g->bound_draw = -1; g->raster_op = -1;
}
GPU_API void GPU_OpEndRenderPass(GPU_Graph* g) {
    REC_GUARD(g);
    GPU_REQUIRE_V(g->in_pass, "GPU_OpEndRenderPass: not inside a render pass");
    close_raster_job(g);
    g->in_pass = nullptr; g->bound_draw = -1;
}
GPU_API void GPU_OpBindDrawParams(GPU_Graph* g, uint32_t idx) {
    REC_GUARD(g);
    GPU_REQUIRE_V(g->in_pass && idx < g->draw_params.size(), "GPU_OpBindDrawParams: bad state / index");
    g->bound_draw = (int)idx;
}

static bool check_plane(Slot* s, GPU_Format f, uint32_t w, uint32_t h, const char* name) {
    GPU_REQUIRE(s && s->tex, false, "lighting pass: \"%s\" is not bound", name);
    GPU_REQUIRE(s->tex->base.format == f && s->tex->base.width == w && s->tex->base.height == h && s->tex->base.layer_count == 1, false,
                "lighting pass: \"%s\" must be a %ux%u 2D texture of format %d", name, w, h, (int)f);
    return true;
}

static bool check_post_plane(Slot* s, GPU_Format f, uint32_t w, uint32_t h, const char* name, const char* fn) {
    GPU_REQUIRE(s && s->tex, false, "%s: \"%s\" is not bound", fn, name);
    GPU_REQUIRE(s->tex->base.format == f && s->tex->base.layer_count == 1 && s->tex->base.depth == 1 && (w == 0 || (s->tex->base.width == w && s->tex->base.height == h)), false,
                "%s: \"%s\" must be a 2D texture of format %d%s", fn, name, (int)f, w ? " with the pass's size" : "");
    return true;
}

// The Op_Shade of a checked full-screen draw: rows [row0, row1) of the pass, or all of them
static void push_shade_op(GPU_Graph* g, Op& op, const DrawParams& dp, uint32_t row0, uint32_t row1, bool explicit_rows, const char* fn) {
    const uint32_t H = g->in_pass->desc.height;
    op.kind = Op_Shade;
    op.gpipe = dp.pipeline; op.set = dp.set; op.pass = g->in_pass;
    op.row0 = explicit_rows ? row0 : 0; op.row1 = explicit_rows ? row1 : H;
    GPU_REQUIRE_V(op.row0 < op.row1 && op.row1 <= H, "%s: rows [%u,%u) outside the %u-row pass", fn, op.row0, op.row1, H);
    g->ops.push_back(op);
}

// taa_resolve.glsl / final_post_process.glsl drawn as the full-screen triangle (render.cpp:1131-1137, 1181-1187)
static void record_post(GPU_Graph* g, const DrawParams& dp, uint32_t row0, uint32_t row1, bool explicit_rows, const char* fn) {
    GPU_RenderPass* rp = g->in_pass;
    uint32_t W = rp->desc.width, H = rp->desc.height;
    GPU_REQUIRE_V(rp->targets.size() == 1 && rp->targets[0].texture && rp->targets[0].mip_level < rp->targets[0].texture->mip_level_count, "%s: the pass needs one colour target", fn);
    TextureImpl* target = (TextureImpl*)rp->targets[0].texture;
    const uint32_t tmip = rp->targets[0].mip_level;
    const bool bloom = is_bloom_kernel(dp.pipeline->kernel);
    GPU_REQUIRE_V(bloom || tmip == 0, "%s: only the bloom passes render into mip levels", fn);
    GPU_REQUIRE_V(mip_dim(target->base.width, tmip) == W && mip_dim(target->base.height, tmip) == H && target->base.layer_count == 1 && target->base.depth == 1,
                  "%s: colour target (mip %u) must be %ux%u", fn, tmip, W, H);
    GPU_DescriptorSet* s = dp.set;
    if (bloom) {                                                              // bloom_*.glsl: TEX0 = BLOOM_INPUT (a texture or one of its mips), int dst_mip_level pushed
        GPU_REQUIRE_V(target->base.format == GPU_Format_RGBA16F, "%s: bloom targets are RGBA16F (render.cpp:742-746)", fn);
        Slot* in = named_slot(s, "TEX0");
        GPU_REQUIRE_V(in && in->tex && in->tex->base.format == GPU_Format_RGBA16F && in->tex->base.layer_count == 1 && in->tex->base.depth == 1, "%s: \"TEX0\" must be an RGBA16F 2D texture", fn);
        uint32_t smip = in->whole ? 0 : in->mip;
        GPU_REQUIRE_V(!(in->tex == target && smip == tmip), "%s: bloom pass reads the level it writes", fn);
        GPU_REQUIRE_V(g->push_size >= 4, "%s: the bloom shaders need their `int dst_mip_level` push constant", fn);
        Op op;
        memcpy(op.push, g->push, g->push_size); op.push_size = g->push_size;
        op.mip = smip; op.mip2 = tmip;
        push_shade_op(g, op, dp, row0, row1, explicit_rows, fn);
        return;
    }
    if (dp.pipeline->kernel == Kernel_TaaResolve) {
        GPU_REQUIRE_V(target->base.format == GPU_Format_RGBA16F || target->base.format == GPU_Format_RGBA32F, "%s: TAA target must be RGBA16F/RGBA32F", fn);
        if (!check_post_plane(named_slot(s, "LIGHTING_RESULT"), GPU_Format_RGBA16F, W, H, "LIGHTING_RESULT", fn)) return;
        if (!check_post_plane(named_slot(s, "GBUFFER_DEPTH"), GPU_Format_D32F_Or_X8D24UN, W, H, "GBUFFER_DEPTH", fn)) return;
        if (!check_post_plane(named_slot(s, "GBUFFER_VELOCITY"), GPU_Format_RG16F, W, H, "GBUFFER_VELOCITY", fn)) return;
        if (!check_post_plane(named_slot(s, "GBUFFER_VELOCITY_PREV"), GPU_Format_RG16F, W, H, "GBUFFER_VELOCITY_PREV", fn)) return;
        if (!check_post_plane(named_slot(s, "PREV_FRAME_RESULT"), GPU_Format_RGBA16F, 0, 0, "PREV_FRAME_RESULT", fn)) return;
        GPU_REQUIRE_V(named_slot(s, "PREV_FRAME_RESULT")->tex != target && named_slot(s, "LIGHTING_RESULT")->tex != target,
                      "%s: the TAA target aliases one of its inputs (the reference ping-pongs taa_output_rt, render.cpp:695-697)", fn);
    } else {
        GPU_REQUIRE_V(target->base.format == GPU_Format_RGBA8UN || target->base.format == GPU_Format_BGRA8UN ||
                      target->base.format == GPU_Format_RGBA16F || target->base.format == GPU_Format_RGBA32F, "%s: unsupported target format %d", fn, (int)target->base.format);
        if (!check_post_plane(named_slot(s, "TEX0"), GPU_Format_RGBA16F, 0, 0, "TEX0", fn)) return;     // final_post_process.glsl:28 BLOOM_RESULT
        GPU_REQUIRE_V(named_slot(s, "TEX0")->tex != target, "%s: target aliases TEX0", fn);
    }
    Op op;
    push_shade_op(g, op, dp, row0, row1, explicit_rows, fn);
}

static void record_shade(GPU_Graph* g, uint32_t row0, uint32_t row1, bool explicit_rows, const char* fn) {
    GPU_REQUIRE_V(g->in_pass && g->bound_draw >= 0, "%s: no draw params bound inside a render pass", fn);
    DrawParams dp = g->draw_params[g->bound_draw];
    GPU_REQUIRE_V(dp.pipeline->pass == g->in_pass, "%s: pipeline was created for a different render pass", fn);
    GPU_REQUIRE_V(dp.set->layout == dp.pipeline->layout, "%s: descriptor set and pipeline use different layouts", fn);
    GPU_RenderPass* rp = g->in_pass;
    uint32_t W = rp->desc.width, H = rp->desc.height;
    if (is_post_kernel(dp.pipeline->kernel)) { record_post(g, dp, row0, row1, explicit_rows, fn); return; }
    GPU_REQUIRE_V(dp.pipeline->kernel == Kernel_Lighting, "%s: unsupported (raster)", fn);
    GPU_REQUIRE_V(rp->targets.size() == 1 && rp->targets[0].texture, "%s: lighting pass needs one colour target", fn);
    TextureImpl* target = (TextureImpl*)rp->targets[0].texture;
    GPU_REQUIRE_V((target->base.format == GPU_Format_RGBA16F || target->base.format == GPU_Format_RGBA32F) &&
                  target->base.width == W && target->base.height == H, "%s: colour target must be %ux%u RGBA16F/RGBA32F", fn, W, H);
    GPU_DescriptorSet* s = dp.set;
    if (!check_plane(named_slot(s, "GBUFFER_BASE_COLOR"), GPU_Format_RGBA8UN, W, H, "GBUFFER_BASE_COLOR")) return;
    if (!check_plane(named_slot(s, "GBUFFER_NORMAL"), GPU_Format_RGBA8UN, W, H, "GBUFFER_NORMAL")) return;
    if (!check_plane(named_slot(s, "GBUFFER_ORM"), GPU_Format_RGBA8UN, W, H, "GBUFFER_ORM")) return;
    if (!check_plane(named_slot(s, "GBUFFER_EMISSIVE"), GPU_Format_RGBA8UN, W, H, "GBUFFER_EMISSIVE")) return;
    if (!check_plane(named_slot(s, "GBUFFER_DEPTH"), GPU_Format_D32F_Or_X8D24UN, W, H, "GBUFFER_DEPTH")) return;
    Slot* gl = named_slot(s, "GLOBALS");
    GPU_REQUIRE_V(gl && gl->buf && gl->buf->base.size >= 552, "%s: \"GLOBALS\" must be a buffer of at least 552 bytes (render.h:122-136)", fn);
    Slot* pre = named_slot(s, "PREFILTERED_ENV_MAP");
    GPU_REQUIRE_V(pre && pre->tex && is_f4_cube(pre->tex), "%s: \"PREFILTERED_ENV_MAP\" must be a square RGBA32F cubemap", fn);
    if (dp.pipeline->shade_flags & GPUX_Shade_SunShadows) {
        Slot* sun = named_slot(s, "SUN_DEPTH_MAP");
        GPU_REQUIRE_V(sun && sun->tex && sun->tex->base.format == GPU_Format_D32F_Or_X8D24UN && sun->tex->base.layer_count == 1 && sun->tex->base.depth == 1,
                      "%s: \"SUN_DEPTH_MAP\" must be a 2D D32F texture (render.cpp:676)", fn);
    }
    if (dp.pipeline->shade_flags & GPUX_Shade_VoxelGI) {
        Slot* grid = named_slot(s, "LIGHTGRID");
        GPU_REQUIRE_V(grid && grid->tex && grid->tex->base.format == GPU_Format_RGBA16F && grid->tex->base.layer_count == 1 &&
                      grid->tex->base.width == grid->tex->base.height && grid->tex->base.width == grid->tex->base.depth && grid->tex->base.width <= 1024,
                      "%s: \"LIGHTGRID\" must be a cubic RGBA16F 3-D texture (render.cpp:678)", fn);
        Slot* prev = named_slot(s, "PREV_FRAME_RESULT");
        GPU_REQUIRE_V(prev && prev->tex && prev->tex->base.format == GPU_Format_RGBA16F && prev->tex->base.layer_count == 1 && prev->tex->base.depth == 1,
                      "%s: \"PREV_FRAME_RESULT\" must be a 2D RGBA16F texture (render.cpp:862 binds bloom_downscale_rt)", fn);
        GPU_REQUIRE_V(prev->tex != target, "%s: PREV_FRAME_RESULT aliases the colour target", fn);
        Slot* lut = named_slot(s, "BRDF_INTEGRATION_MAP");
        GPU_REQUIRE_V(lut && lut->tex && lut->tex->base.format == GPU_Format_RG16F && lut->tex->base.width == lut->tex->base.height,
                      "%s: \"BRDF_INTEGRATION_MAP\" must be a square RG16F texture", fn);
    }
    Op op;
    if (dp.pipeline->shade_flags & GPUX_Shade_SH9Irradiance) {                // the 27 coefficients in place of TEX_IRRADIANCE_MAP
        BufferImpl* coef = dp.pipeline->sh9_buf;
        const uint32_t off = dp.pipeline->sh9_offset;
        GPU_REQUIRE_V(dp.pipeline->shade_flags & GPUX_Shade_IBL, "%s: GPUX_Shade_SH9Irradiance needs GPUX_Shade_IBL", fn);
        GPU_REQUIRE_V(coef, "%s: GPUX_Shade_SH9Irradiance without a coefficient buffer (GPUX_SetShadeSH9)", fn);
        GPU_REQUIRE_V((off % 8) == 0, "%s: SH9 coefficient offset %u is not a multiple of 8", fn, off);
        GPU_REQUIRE_V((uint64_t)off + 27 * sizeof(double) <= coef->base.size, "%s: SH9 coefficient buffer too small (%u bytes for 216 at offset %u)", fn, coef->base.size, off);
        op.buf = coef; op.off_a = off;
    }
    if (dp.pipeline->shade_flags & GPUX_Shade_IBL) {
        Slot* irr = named_slot(s, "TEX_IRRADIANCE_MAP");
        GPU_REQUIRE_V(op.buf || (irr && irr->tex && is_f4_cube(irr->tex)), "%s: \"TEX_IRRADIANCE_MAP\" must be a square RGBA32F cubemap", fn);
        Slot* lut = named_slot(s, "BRDF_INTEGRATION_MAP");
        GPU_REQUIRE_V(lut && lut->tex && lut->tex->base.format == GPU_Format_RG16F && lut->tex->base.width == lut->tex->base.height,
                      "%s: \"BRDF_INTEGRATION_MAP\" must be a square RG16F texture", fn);
    }
    push_shade_op(g, op, dp, row0, row1, explicit_rows, fn);
}

GPU_API void GPU_OpDraw(GPU_Graph* g, uint32_t vertex_count, uint32_t instance_count, uint32_t first_vertex, uint32_t first_instance) {
    REC_GUARD(g);
    const RasterKind* rk = bound_raster_row(g);
    if (rk && !rk->indexed) { record_raster_draw(g, g->draw_params[(size_t)g->bound_draw], vertex_count, instance_count, first_vertex, 0, __func__); return; }   // the shader never reads gl_InstanceIndex
    GPU_REQUIRE_V(vertex_count == 3 && instance_count == 1 && first_vertex == 0 && first_instance == 0,
                  "GPU_OpDraw: unsupported (raster): only the full-screen triangle GPU_OpDraw(3,1,0,0) of the lighting pass is implemented");
    record_shade(g, 0, 0, false, __func__);
}
GPU_API void GPUX_OpDrawRows(GPU_Graph* g, uint32_t row0, uint32_t row1) { REC_GUARD(g); record_shade(g, row0, row1, true, __func__); }
GPU_API void GPU_OpDrawIndexed(GPU_Graph* g, uint32_t index_count, uint32_t instance_count, uint32_t first_index, uint32_t vertex_offset, uint32_t first_instance) {
    (void)first_instance;                                                     // the shader never reads gl_InstanceIndex
    REC_GUARD(g);
    const RasterKind* rk = bound_raster_row(g);
    GPU_REQUIRE_V(rk && rk->indexed, "GPU_OpDrawIndexed: unsupported (raster): only the sun depth pass (sun_depth_pass.glsl) and the geometry pass (geometry_pass.glsl) draw indexed triangles");
    record_raster_draw(g, g->draw_params[(size_t)g->bound_draw], index_count, instance_count, first_index, vertex_offset, __func__);
}
GPU_API void GPU_OpBindVertexBuffer(GPU_Graph* g, GPU_Buffer* b) {
    REC_GUARD(g);
    GPU_REQUIRE_V(b, "GPU_OpBindVertexBuffer: NULL buffer");
    g->vertex_buffer = (BufferImpl*)b;
}
GPU_API void GPU_OpBindIndexBuffer(GPU_Graph* g, GPU_Buffer* b) {
    REC_GUARD(g);
    GPU_REQUIRE_V(b, "GPU_OpBindIndexBuffer: NULL buffer");
    g->index_buffer = (BufferImpl*)b;
}
GPU_API uint64_t GPUX_RasterRejectedTriangles(void) {
    uint64_t v = G.raster_rejected_base;
    unsigned long long d = 0;
    if (G.init && G.raster_rejected && hipMemcpy(&d, G.raster_rejected, 8, hipMemcpyDeviceToHost) == hipSuccess) v += d;
    return v;
}

GPU_API uint64_t GPUX_VoxelizeFragments(void) {
    unsigned long long d = 0;
    if (G.init && G.raster_rejected && hipMemcpy(&d, G.raster_rejected + 1, 8, hipMemcpyDeviceToHost) != hipSuccess) d = 0;
    return d;
}

// ---- transfers ----
GPU_API void GPU_OpCopyBufferToBuffer(GPU_Graph* g, GPU_Buffer* src, GPU_Buffer* dst, uint32_t dst_offset, uint32_t src_offset, uint32_t size) {
    REC_GUARD(g);
    GPU_REQUIRE_V(g->in_pass == nullptr, "GPU_OpCopyBufferToBuffer: inside a render pass");
    GPU_REQUIRE_V(src && dst && (uint64_t)src_offset + size <= src->size && (uint64_t)dst_offset + size <= dst->size, "GPU_OpCopyBufferToBuffer: range out of bounds");
    Op op; op.kind = Op_CopyB2B; op.name = "copy.buffer_to_buffer";
    op.buf = (BufferImpl*)src; op.buf2 = (BufferImpl*)dst; op.off_a = src_offset; op.off_b = dst_offset; op.size = size;
    g->ops.push_back(op);
}
GPU_API void GPU_OpCopyBufferToTexture(GPU_Graph* g, GPU_Buffer* src, GPU_Texture* dst, uint32_t first_layer, uint32_t layer_count, uint32_t mip) {
    REC_GUARD(g);
    GPU_REQUIRE_V(g->in_pass == nullptr, "GPU_OpCopyBufferToTexture: inside a render pass");
    GPU_REQUIRE_V(src && dst && mip < dst->mip_level_count && layer_count > 0 && first_layer + layer_count <= dst->layer_count, "GPU_OpCopyBufferToTexture: bad subresource");
    uint64_t per_layer = GPUX_TextureMipBytes(dst, mip) / dst->layer_count;
    GPU_REQUIRE_V(per_layer * layer_count <= src->size, "GPU_OpCopyBufferToTexture: buffer too small (%u < %llu)", src->size, (unsigned long long)(per_layer * layer_count));
    Op op; op.kind = Op_CopyB2T; op.name = "copy.buffer_to_texture";
    op.buf = (BufferImpl*)src; op.tex = (TextureImpl*)dst; op.mip = mip; op.layer0 = first_layer; op.layer_count = layer_count; op.off_a = 0;
    g->ops.push_back(op);
}
GPU_API void GPUX_OpCopyBufferToTextureMip(GPU_Graph* g, GPU_Buffer* src, uint32_t src_offset, GPU_Texture* dst, uint32_t mip) {
    REC_GUARD(g);
    GPU_REQUIRE_V(src && dst && mip < dst->mip_level_count, "GPUX_OpCopyBufferToTextureMip: bad arguments");
    GPU_REQUIRE_V((uint64_t)src_offset + GPUX_TextureMipBytes(dst, mip) <= src->size, "GPUX_OpCopyBufferToTextureMip: buffer too small");
    Op op; op.kind = Op_CopyB2T; op.name = "copy.buffer_to_texture";
    op.buf = (BufferImpl*)src; op.tex = (TextureImpl*)dst; op.mip = mip; op.layer0 = 0; op.layer_count = dst->layer_count; op.off_a = src_offset;
    g->ops.push_back(op);
}
static void record_t2b(GPU_Graph* g, GPU_Texture* src, uint32_t mip, GPU_Buffer* dst, uint32_t dst_offset, const char* fn) {
    GPU_REQUIRE_V(g->in_pass == nullptr, "%s: inside a render pass", fn);
    GPU_REQUIRE_V(src && dst && mip < src->mip_level_count, "%s: bad arguments", fn);
    GPU_REQUIRE_V((uint64_t)dst_offset + GPUX_TextureMipBytes(src, mip) <= dst->size, "%s: buffer too small (%u bytes for %llu)", fn, dst->size,
                  (unsigned long long)GPUX_TextureMipBytes(src, mip));
    Op op; op.kind = Op_CopyT2B; op.name = "copy.texture_to_buffer";
    op.tex = (TextureImpl*)src; op.mip = mip; op.buf = (BufferImpl*)dst; op.off_b = dst_offset;
    g->ops.push_back(op);
}
GPU_API void GPU_OpCopyTextureToBuffer(GPU_Graph* g, GPU_Texture* src, GPU_Buffer* dst) { REC_GUARD(g); record_t2b(g, src, 0, dst, 0, __func__); }   // mip 0 only (gpu_vulkan.c:2948)
GPU_API void GPUX_OpCopyTextureMipToBuffer(GPU_Graph* g, GPU_Texture* src, uint32_t mip, GPU_Buffer* dst, uint32_t off) { REC_GUARD(g); record_t2b(g, src, mip, dst, off, __func__); }

// K15 test accessor: one level of a BC texture's decoded image (RGBA8UN, tight rows) -> buffer
GPU_API void GPUX_OpCopyDecodedTextureMipToBuffer(GPU_Graph* g, GPU_Texture* src, uint32_t mip, GPU_Buffer* dst, uint32_t dst_offset) {
    REC_GUARD(g);
    const char* fn = "GPUX_OpCopyDecodedTextureMipToBuffer";
    GPU_REQUIRE_V(g->in_pass == nullptr, "%s: inside a render pass", fn);
    GPU_REQUIRE_V(src && dst && mip < src->mip_level_count, "%s: bad arguments", fn);
    TextureImpl* t = (TextureImpl*)src;
    GPU_REQUIRE_V(is_bc_format(src->format) && t->decoded, "%s: the texture has no decoded image (only 2-D BC1 / BC3 / BC5 textures do)", fn);
    const uint64_t bytes = (uint64_t)mip_dim(src->width, mip) * mip_dim(src->height, mip) * 4;
    GPU_REQUIRE_V((uint64_t)dst_offset + bytes <= dst->size, "%s: buffer too small (%u bytes for %llu)", fn, dst->size, (unsigned long long)bytes);
    Op op; op.kind = Op_CopyDecodedT2B; op.name = "copy.decoded_texture_to_buffer";
    op.tex = t; op.mip = mip; op.buf = (BufferImpl*)dst; op.off_b = dst_offset; op.size = bytes;
    g->ops.push_back(op);
}

// ---- K17: SH9 projection of a cube level into a buffer, and the irradiance cube of nine coefficients ----
// op.tex / op.mip = the cube level, op.buf / op.off_b = the 27 doubles, faces [face0, face1) x rows [row0, row1)
static bool record_sh9(GPU_Graph* g, OpKind kind, const char* name, GPU_Texture* cube, uint32_t mip, GPU_Buffer* buf, uint32_t offset, const char* fn) {
    GPU_REQUIRE(g->in_pass == nullptr, false, "%s: inside a render pass", fn);
    GPU_REQUIRE(cube && buf && mip < cube->mip_level_count, false, "%s: bad arguments", fn);
    GPU_REQUIRE(is_f4_cube((TextureImpl*)cube), false, "%s: the texture must be a square RGBA32F cubemap", fn);
    GPU_REQUIRE((offset % 8) == 0, false, "%s: buffer offset %u is not a multiple of 8", fn, offset);
    GPU_REQUIRE((uint64_t)offset + 27 * sizeof(double) <= buf->size, false, "%s: buffer too small (%u bytes for 216 at offset %u)", fn, buf->size, offset);
    Op op; op.kind = kind; op.name = name;
    op.tex = (TextureImpl*)cube; op.mip = mip; op.buf = (BufferImpl*)buf; op.off_b = offset;
    op.face0 = 0; op.face1 = 6; op.row0 = 0; op.row1 = mip_dim(cube->width, mip);
    g->ops.push_back(op);
    return true;
}
GPU_API void GPUX_OpProjectSH9(GPU_Graph* g, GPU_Texture* cube, uint32_t mip, uint32_t face0, uint32_t face1, uint32_t row0, uint32_t row1,
                               GPU_Buffer* dst, uint32_t dst_offset) {
    REC_GUARD(g);
    const char* fn = "GPUX_OpProjectSH9";
    GPU_REQUIRE_V(cube && mip < cube->mip_level_count, "%s: bad arguments", fn);
    const uint32_t n = mip_dim(cube->width, mip);
    GPU_REQUIRE_V(face0 < face1 && face1 <= 6 && row0 < row1 && row1 <= n, "%s: empty or out-of-range faces [%u, %u) x rows [%u, %u) of a %u^2 level", fn,
                  face0, face1, row0, row1, n);
    GPU_REQUIRE_V(n <= 16384, "%s: levels above 16384^2 are not implemented", fn);
    if (!record_sh9(g, Op_ProjectSH9, "K17.sh_project", cube, mip, dst, dst_offset, fn)) return;
    { Op& op = g->ops.back(); op.face0 = face0; op.face1 = face1; op.row0 = row0; op.row1 = row1; }
    // the partials' scratch grows here, not at submit: nothing allocates inside a captured submission, and the graph is idle while it records
    const size_t need = pbrk_sh9_scratch_bytes((int)n);
    if (need > g->sh_scratch_bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, need) != hipSuccess) { (void)hipGetLastError(); g->ops.pop_back(); gpu_fail("%s: allocation of the partials' scratch (%zu bytes) failed", fn, need); return; }
        (void)hipFree(g->sh_scratch);
        g->sh_scratch = p; g->sh_scratch_bytes = need;
    }
}
GPU_API void GPUX_OpIrradianceFromSH9(GPU_Graph* g, GPU_Buffer* src, uint32_t src_offset, GPU_Texture* irradiance_cube, uint32_t mip) {
    REC_GUARD(g);
    const char* fn = "GPUX_OpIrradianceFromSH9";
    GPU_REQUIRE_V(irradiance_cube && mip < irradiance_cube->mip_level_count, "%s: bad arguments", fn);
    GPU_REQUIRE_V(mip_dim(irradiance_cube->width, mip) <= 16384, "%s: levels above 16384^2 are not implemented", fn);
    record_sh9(g, Op_IrradianceSH9, "K17.sh_irradiance", irradiance_cube, mip, src, src_offset, fn);
}

// ---- K18: one level of an RGBA32F / RGBA16F texture -> BC6H_UF16 blocks in a buffer ----
static int bc6h_source_format(GPU_Format f) { return f == GPU_Format_RGBA32F ? PBRK_FMT_RGBA32F : f == GPU_Format_RGBA16F ? PBRK_FMT_RGBA16F : -1; }
GPU_API uint64_t GPUX_BC6HMipBytes(const GPU_Texture* t, uint32_t mip) {
    if (!t || mip >= t->mip_level_count || t->depth != 1 || bc6h_source_format(t->format) < 0) return 0;
    return pbrk_bc6h_level_bytes((int)mip_dim(t->width, mip), (int)mip_dim(t->height, mip), (int)t->layer_count);
}
// op.tex / op.mip = the source level (all layers), op.buf / op.off_b = the blocks, op.size = their bytes, op.quality = the level
static void record_bc6h_encode(GPU_Graph* g, GPU_Texture* src, uint32_t mip, GPU_Buffer* dst, uint32_t dst_offset, uint32_t quality, const char* fn) {
    GPU_REQUIRE_V(g && !g->submitted, "%s: graph is NULL or already submitted (call GPU_GraphWait first)", fn);
    GPU_REQUIRE_V(g->in_pass == nullptr, "%s: inside a render pass", fn);
    GPU_REQUIRE_V(src && dst && mip < src->mip_level_count, "%s: bad arguments", fn);
    GPU_REQUIRE_V(quality == GPUX_BC6H_OneRegion || quality == GPUX_BC6H_TwoRegions, "%s: quality %u is neither GPUX_BC6H_OneRegion (0) nor GPUX_BC6H_TwoRegions (1)", fn, quality);
    GPU_REQUIRE_V(bc6h_source_format(src->format) >= 0 && src->depth == 1, "%s: the source must be a 2-D or cube RGBA32F / RGBA16F texture", fn);
    GPU_REQUIRE_V(mip_dim(src->width, mip) <= 16384 && mip_dim(src->height, mip) <= 16384, "%s: levels above 16384 a side are not implemented", fn);
    GPU_REQUIRE_V((dst_offset % 16) == 0, "%s: buffer offset %u is not a multiple of 16", fn, dst_offset);
    const uint64_t bytes = GPUX_BC6HMipBytes(src, mip);
    GPU_REQUIRE_V((uint64_t)dst_offset + bytes <= dst->size, "%s: buffer too small (%u bytes for %llu at offset %u)", fn, dst->size, (unsigned long long)bytes, dst_offset);
    Op op; op.kind = Op_EncodeBC6H; op.name = quality == GPUX_BC6H_TwoRegions ? "K18.bc6h_encode2" : "K18.bc6h_encode";
    op.tex = (TextureImpl*)src; op.mip = mip; op.quality = quality; op.buf = (BufferImpl*)dst; op.off_b = dst_offset; op.size = bytes;
    g->ops.push_back(op);
}
GPU_API void GPUX_OpEncodeBC6H(GPU_Graph* g, GPU_Texture* src, uint32_t mip, GPU_Buffer* dst, uint32_t dst_offset) {
    record_bc6h_encode(g, src, mip, dst, dst_offset, GPUX_BC6H_OneRegion, "GPUX_OpEncodeBC6H");
}
GPU_API void GPUX_OpEncodeBC6HEx(GPU_Graph* g, GPU_Texture* src, uint32_t mip, GPU_Buffer* dst, uint32_t dst_offset, uint32_t quality) {
    record_bc6h_encode(g, src, mip, dst, dst_offset, quality, "GPUX_OpEncodeBC6HEx");
}
// K19: the way back.  op.buf / op.off_a = the blocks, op.tex / op.mip = the level written (all layers), op.size = the blocks' bytes
GPU_API void GPUX_OpDecodeBC6H(GPU_Graph* g, GPU_Buffer* src, uint32_t src_offset, GPU_Texture* dst, uint32_t mip) {
    REC_GUARD(g);
    const char* fn = "GPUX_OpDecodeBC6H";
    GPU_REQUIRE_V(g->in_pass == nullptr, "%s: inside a render pass", fn);
    GPU_REQUIRE_V(src && dst && mip < dst->mip_level_count, "%s: bad arguments", fn);
    GPU_REQUIRE_V(bc6h_source_format(dst->format) >= 0 && dst->depth == 1, "%s: the target must be a 2-D or cube RGBA32F / RGBA16F texture", fn);
    GPU_REQUIRE_V(mip_dim(dst->width, mip) <= 16384 && mip_dim(dst->height, mip) <= 16384, "%s: levels above 16384 a side are not implemented", fn);
    GPU_REQUIRE_V((src_offset % 16) == 0, "%s: buffer offset %u is not a multiple of 16", fn, src_offset);
    const uint64_t bytes = GPUX_BC6HMipBytes(dst, mip);
    GPU_REQUIRE_V((uint64_t)src_offset + bytes <= src->size, "%s: buffer too small (%u bytes for %llu at offset %u)", fn, src->size, (unsigned long long)bytes, src_offset);
    Op op; op.kind = Op_DecodeBC6H; op.name = "K19.bc6h_decode";
    op.buf = (BufferImpl*)src; op.off_a = src_offset; op.tex = (TextureImpl*)dst; op.mip = mip; op.size = bytes;
    g->ops.push_back(op);
}

// The table of an op that brings one (K20, K21, K22) is allocated and uploaded when the op is recorded, not at submit: nothing allocates
// inside a submission, and the graph is idle while it records.  A slot of an earlier recording is used again; a slot in use is never
// touched, so the ops recorded so far keep theirs.  NULL after one error.
static const void* upload_op_table(GPU_Graph* g, const void* data, size_t bytes, const char* fn) {
    if (g->pano_used == g->pano.size()) g->pano.push_back(GPU_Graph::PanoTable());
    GPU_Graph::PanoTable& slot = g->pano[g->pano_used];
    if (slot.bytes < bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); gpu_fail("%s: allocation of the op's table (%zu bytes) failed", fn, bytes); return nullptr; }
        (void)hipFree(slot.dev);
        slot.dev = p; slot.bytes = bytes;
    }
    if (hipMemcpy(slot.dev, data, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); gpu_fail("%s: upload of the op's table failed", fn); return nullptr; }
    ++g->pano_used;
    return slot.dev;
}

// ---- K20: one level of an RGBA32F cube -> one level of a 2-D RGBA32F / RGBA16F texture as a lat-long panorama ----
// The directions of a w x h panorama, from the entries pano_fill_table writes: what the kernel forms from the uploaded table
static void pano_directions(const double* table, int w, int h, float* xyz) {
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) pano_dir(table + 2 * x, table + 2 * (w + y), xyz + 3 * ((size_t)y * w + x));
}
GPU_API int GPUX_PanoramaDirections(uint32_t width, uint32_t height, float* xyz) {
    if (!xyz || width < 1 || height < 1 || width > PANO_MAX_EXTENT || height > PANO_MAX_EXTENT) return 1;
    std::vector<double> table(2 * ((size_t)width + height));
    pano_fill_table((int)width, (int)height, table.data());
    pano_directions(table.data(), (int)width, (int)height, xyz);
    return 0;
}
// op.tex / op.mip = the cube level, op.tex2 / op.mip2 = the panorama, op.pano_table = its table on the device
GPU_API void GPUX_OpCubeToPanorama(GPU_Graph* g, GPU_Texture* cube, uint32_t src_mip, GPU_Texture* dst, uint32_t dst_mip) {
    REC_GUARD(g);
    const char* fn = "GPUX_OpCubeToPanorama";
    GPU_REQUIRE_V(g->in_pass == nullptr, "%s: inside a render pass", fn);
    GPU_REQUIRE_V(cube && dst && src_mip < cube->mip_level_count && dst_mip < dst->mip_level_count, "%s: bad arguments", fn);
    GPU_REQUIRE_V(is_f4_cube((TextureImpl*)cube), "%s: the source must be a square RGBA32F cubemap", fn);
    GPU_REQUIRE_V((dst->format == GPU_Format_RGBA32F || dst->format == GPU_Format_RGBA16F) && dst->depth == 1 && dst->layer_count == 1,
                  "%s: the target must be a 2-D RGBA32F / RGBA16F texture", fn);
    const uint32_t n = mip_dim(cube->width, src_mip), w = mip_dim(dst->width, dst_mip), h = mip_dim(dst->height, dst_mip);
    GPU_REQUIRE_V(n <= PANO_MAX_EXTENT && w <= PANO_MAX_EXTENT && h <= PANO_MAX_EXTENT, "%s: levels above 16384 a side are not implemented", fn);
    std::vector<double> table(2 * ((size_t)w + h));
    pano_fill_table((int)w, (int)h, table.data());
    const void* dev = upload_op_table(g, table.data(), table.size() * sizeof(double), fn);
    if (!dev) return;
    Op op; op.kind = Op_CubeToPanorama; op.name = "K20.cube_to_panorama";
    op.tex = (TextureImpl*)cube; op.mip = src_mip; op.tex2 = (TextureImpl*)dst; op.mip2 = dst_mip; op.pano_table = dev;
    g->ops.push_back(op);
}

// ---- K21: one level of an RGBA32F cube from another RGBA32F cube by GGX importance sampling with filtered lookups ----
static bool ggx_args_ok(float roughness, uint32_t sample_count, float lod_bias) {
    return roughness > 0.0f && roughness <= 1.0f && sample_count >= 1 && sample_count <= PGGX_MAX_SAMPLES && isfinite(lod_bias);
}
GPU_API int GPUX_PrefilterGGXSamples(float roughness, uint32_t sample_count, uint32_t src_size, uint32_t src_levels, float lod_bias,
                                     float* xyz_lod, uint32_t* kept, float* wsum) {
    if (!xyz_lod || !kept || !wsum || !ggx_args_ok(roughness, sample_count, lod_bias) || src_size < 1 || src_size > 16384 ||
        src_levels < 1 || src_levels > (uint32_t)pbrk_mip_count((int)src_size, (int)src_size)) return 1;
    *kept = pggx_fill_table(roughness, sample_count, src_size, src_levels, lod_bias, xyz_lod, wsum);
    return 0;
}
// op.tex = the source cube, op.tex2 / op.mip2 = the target level, faces [face0, face1) x rows [row0, row1), op.ggx_* = its table
GPU_API void GPUX_OpPrefilterGGX(GPU_Graph* g, GPU_Texture* env_cube, GPU_Texture* dst_cube, uint32_t dst_mip, float roughness,
                                 uint32_t sample_count, float lod_bias, uint32_t face0, uint32_t face1, uint32_t row0, uint32_t row1) {
    REC_GUARD(g);
    const char* fn = "GPUX_OpPrefilterGGX";
    GPU_REQUIRE_V(g->in_pass == nullptr, "%s: inside a render pass", fn);
    GPU_REQUIRE_V(env_cube && dst_cube && env_cube != dst_cube && dst_mip < dst_cube->mip_level_count, "%s: bad arguments (NULL, the source as its own target, or a mip out of range)", fn);
    GPU_REQUIRE_V(is_f4_cube((TextureImpl*)env_cube) && is_f4_cube((TextureImpl*)dst_cube), "%s: source and target must be square RGBA32F cubemaps", fn);
    GPU_REQUIRE_V(ggx_args_ok(roughness, sample_count, lod_bias), "%s: roughness %g outside (0, 1], %u samples outside 1 .. %d, or lod_bias %g not finite", fn,
                  (double)roughness, sample_count, PGGX_MAX_SAMPLES, (double)lod_bias);
    const uint32_t size = mip_dim(dst_cube->width, dst_mip), W = env_cube->width, levels = env_cube->mip_level_count;
    GPU_REQUIRE_V(face0 < face1 && face1 <= 6 && row0 < row1 && row1 <= size, "%s: empty or out-of-range faces [%u, %u) x rows [%u, %u) of a %u^2 level", fn,
                  face0, face1, row0, row1, size);
    GPU_REQUIRE_V(W <= 16384 && size <= 16384, "%s: levels above 16384 a side are not implemented", fn);
    // the kernel's form of the table: per kept sample {l.x, l.y, l.z, f} and the two levels it blends, as offset and size inside the
    // bordered twin.  floorf and the difference are exact, so f is the contract's lod - floorf(lod)
    std::vector<float> e(4 * (size_t)sample_count);
    float wsum = 0.0f;
    const uint32_t kept = pggx_fill_table(roughness, sample_count, W, levels, lod_bias, e.data(), &wsum);
    std::vector<uint32_t> table(8 * (size_t)kept + 8);                        // never empty: a table of no entries still has a slot
    for (uint32_t i = 0; i < kept; ++i) {
        const float lod = e[4 * i + 3], fl = floorf(lod), f = lod - fl;
        const uint32_t l0 = (uint32_t)fl, l1 = l0 + 1 < levels ? l0 + 1 : levels - 1;
        uint32_t* t = &table[8 * (size_t)i];
        memcpy(t, &e[4 * i], 12); memcpy(t + 3, &f, 4);
        t[4] = (uint32_t)pbrk_bordered_level_offset((int)W, (int)l0); t[5] = mip_dim(W, l0);
        t[6] = (uint32_t)pbrk_bordered_level_offset((int)W, (int)l1); t[7] = mip_dim(W, l1);
    }
    const void* dev = upload_op_table(g, table.data(), table.size() * sizeof(uint32_t), fn);
    if (!dev) return;
    Op op; op.kind = Op_PrefilterGGX; op.name = "K21.prefilter_ggx.mip" + std::to_string(dst_mip);
    op.tex = (TextureImpl*)env_cube; op.tex2 = (TextureImpl*)dst_cube; op.mip2 = dst_mip;
    op.face0 = face0; op.face1 = face1; op.row0 = row0; op.row1 = row1;
    op.ggx_table = dev; op.ggx_kept = kept; op.ggx_wsum = wsum;
    g->ops.push_back(op);
}

// ---- K22: rows of a 2-D RG16F / RG32F / RGBA32F texture as the GGX split-sum BRDF LUT ----
GPU_API int GPUX_BrdfLutGGXSamples(uint32_t sample_count, float* xi_cos_sin) {
    if (!xi_cos_sin || sample_count < 1 || sample_count > BLG_MAX_SAMPLES) return 1;
    blg_fill_table(sample_count, xi_cos_sin);
    return 0;
}
// op.tex = the map, rows [row0, row1), op.lut_* = its table, count and visibility term
GPU_API void GPUX_OpBrdfLutGGX(GPU_Graph* g, GPU_Texture* lut_tex, uint32_t sample_count, uint32_t visibility, uint32_t row0, uint32_t row1) {
    REC_GUARD(g);
    const char* fn = "GPUX_OpBrdfLutGGX";
    GPU_REQUIRE_V(g->in_pass == nullptr, "%s: inside a render pass", fn);
    GPU_REQUIRE_V(lut_tex, "%s: the texture is NULL", fn);
    GPU_REQUIRE_V((lut_tex->format == GPU_Format_RG16F || lut_tex->format == GPU_Format_RG32F || lut_tex->format == GPU_Format_RGBA32F) &&
                  !(lut_tex->flags & GPU_TextureFlag_Cubemap) && lut_tex->layer_count == 1 && lut_tex->depth == 1,
                  "%s: the target must be a 2-D RG16F / RG32F / RGBA32F texture", fn);
    GPU_REQUIRE_V(lut_tex->width <= BLG_MAX_EXTENT && lut_tex->height <= BLG_MAX_EXTENT, "%s: a %u x %u map is above %d a side", fn,
                  lut_tex->width, lut_tex->height, BLG_MAX_EXTENT);
    GPU_REQUIRE_V(sample_count >= 1 && sample_count <= BLG_MAX_SAMPLES, "%s: %u samples outside 1 .. %d", fn, sample_count, BLG_MAX_SAMPLES);
    GPU_REQUIRE_V(visibility == GPUX_BrdfLut_SmithSchlick || visibility == GPUX_BrdfLut_SmithCorrelated, "%s: unknown visibility term %u", fn, visibility);
    GPU_REQUIRE_V(row0 < row1 && row1 <= lut_tex->height, "%s: empty or out-of-range rows [%u, %u) of a %u x %u map", fn, row0, row1,
                  lut_tex->width, lut_tex->height);
    std::vector<float> table(3 * (size_t)sample_count);
    blg_fill_table(sample_count, table.data());
    const void* dev = upload_op_table(g, table.data(), table.size() * sizeof(float), fn);
    if (!dev) return;
    Op op; op.kind = Op_BrdfLutGGX; op.name = "K22.brdf_lut_ggx";
    op.tex = (TextureImpl*)lut_tex; op.row0 = row0; op.row1 = row1;
    op.lut_table = dev; op.lut_samples = sample_count; op.lut_visibility = visibility;
    g->ops.push_back(op);
}

GPU_API void GPU_OpGenerateMipmaps(GPU_Graph* g, GPU_Texture* tex) {
    REC_GUARD(g);
    GPU_REQUIRE_V(tex, "GPU_OpGenerateMipmaps: NULL texture");
    TextureImpl* t = (TextureImpl*)tex;
    GPU_REQUIRE_V(is_f4_cube(t) || is_rgba8_pow2(t), "GPU_OpGenerateMipmaps: implemented for RGBA32F cubemaps and power-of-two 2-D RGBA8UN textures only");
    Op op; op.kind = Op_MipGen; op.name = "K2.mip_chain"; op.tex = t;
    g->ops.push_back(op);
}
GPU_API void GPU_OpBlit(GPU_Graph* g, const GPU_OpBlitInfo* info) {
    REC_GUARD(g);
    GPU_REQUIRE_V(g->in_pass == nullptr, "GPU_OpBlit: inside a render pass");                                        // gpu_vulkan.c:2787
    GPU_REQUIRE_V(info && info->src_texture && info->dst_texture, "GPU_OpBlit: NULL argument");
    const GPU_Texture* s = info->src_texture; const GPU_Texture* d = info->dst_texture;
    GPU_REQUIRE_V(!is_bc_format(s->format) && !is_bc_format(d->format), "GPU_OpBlit: block-compressed textures cannot be blitted (copy their levels through a buffer)");
    if (s == d) GPU_REQUIRE_V(info->dst_mip_level != info->src_mip_level || info->src_layer != info->dst_layer, "GPU_OpBlit: blit of a subresource onto itself");   // :2792
    GPU_REQUIRE_V(info->src_mip_level < s->mip_level_count && info->dst_mip_level < d->mip_level_count && info->src_layer < s->layer_count && info->dst_layer < d->layer_count,
                  "GPU_OpBlit: bad subresource");
    {   // whole-subresource 1:1 blit between equal formats (render.cpp:1158-1163: TAA result -> bloom_upscale_rt mip 0): a copy under either filter
        uint32_t sw1 = mip_dim(s->width, info->src_mip_level), sh1 = mip_dim(s->height, info->src_mip_level);
        uint32_t dw1 = mip_dim(d->width, info->dst_mip_level), dh1 = mip_dim(d->height, info->dst_mip_level);
        bool whole = info->src_area[0].x == 0 && info->src_area[0].y == 0 && info->dst_area[0].x == 0 && info->dst_area[0].y == 0 &&
                     (uint32_t)info->src_area[1].x == sw1 && (uint32_t)info->src_area[1].y == sh1 && (uint32_t)info->dst_area[1].x == dw1 && (uint32_t)info->dst_area[1].y == dh1;
        if (whole && sw1 == dw1 && sh1 == dh1 && s->format == d->format && s->depth == 1 && d->depth == 1) {
            Op op; op.kind = Op_Blit; op.name = "blit_1to1";
            op.tex = (TextureImpl*)s; op.tex2 = (TextureImpl*)d; op.mip = info->src_mip_level; op.mip2 = info->dst_mip_level;
            op.layer0 = info->src_layer; op.layer2 = info->dst_layer;
            op.size = (uint64_t)sw1 * sh1 * ((TextureImpl*)s)->texel_bytes;
            g->ops.push_back(op);
            return;
        }
    }
    GPU_REQUIRE_V(s->format == GPU_Format_RGBA32F && d->format == GPU_Format_RGBA32F && info->filter == GPU_Filter_Linear, "GPU_OpBlit: RGBA32F linear blits only");
    GPU_REQUIRE_V(info->src_mip_level < s->mip_level_count && info->dst_mip_level < d->mip_level_count && info->src_layer < s->layer_count && info->dst_layer < d->layer_count,
                  "GPU_OpBlit: bad subresource");
    uint32_t sw = mip_dim(s->width, info->src_mip_level), sh = mip_dim(s->height, info->src_mip_level);
    uint32_t dw = mip_dim(d->width, info->dst_mip_level), dh = mip_dim(d->height, info->dst_mip_level);
    bool full = info->src_area[0].x == 0 && info->src_area[0].y == 0 && info->dst_area[0].x == 0 && info->dst_area[0].y == 0 &&
                (uint32_t)info->src_area[1].x == sw && (uint32_t)info->src_area[1].y == sh && (uint32_t)info->dst_area[1].x == dw && (uint32_t)info->dst_area[1].y == dh;
    GPU_REQUIRE_V(full && s->depth == 1 && d->depth == 1, "GPU_OpBlit: only whole-subresource 2-D blits are implemented");
    Op op; op.kind = Op_Blit;
    // exact 2:1 square blits (every level of a power-of-two mip chain, gpu_vulkan.c:1458-1483) are the 2x2 box; anything else is the
    // linear resample of oracle/pbr_oracle.c A2 (odd levels of faces that are not a power of two: 125 -> 62)
    op.name = (sw == sh && dw == dh && sw == 2 * dw) ? "K2.blit_2to1" : "K2.blit_linear";
    op.tex = (TextureImpl*)s; op.tex2 = (TextureImpl*)d; op.mip = info->src_mip_level; op.mip2 = info->dst_mip_level;
    op.layer0 = info->src_layer; op.layer2 = info->dst_layer;
    g->ops.push_back(op);
}
static void record_clear(GPU_Graph* g, GPU_Texture* dst, uint32_t mip, int mode, const float* f, const uint32_t* u, const char* fn) {
    GPU_REQUIRE_V(g->in_pass == nullptr, "%s: inside a render pass", fn);
    GPU_REQUIRE_V(dst && (mip == GPU_MIP_LEVEL_ALL || mip < dst->mip_level_count), "%s: bad texture / mip", fn);
    GPU_REQUIRE_V(!is_bc_format(dst->format), "%s: block-compressed textures cannot be cleared (copy their levels in from a buffer)", fn);
    Op op; op.kind = Op_Clear; op.name = "clear"; op.tex = (TextureImpl*)dst; op.mip = mip; op.clear_mode = mode;
    for (int i = 0; i < 4; ++i) { op.clear[i] = f ? f[i] : 0.0f; op.cleari[i] = u ? u[i] : 0; }
    g->ops.push_back(op);
}
GPU_API void GPU_OpClearColorF(GPU_Graph* g, GPU_Texture* dst, uint32_t mip, float r, float gg, float b, float a) {
    REC_GUARD(g); float f[4] = {r, gg, b, a}; record_clear(g, dst, mip, 0, f, nullptr, __func__);
}
GPU_API void GPU_OpClearColorI(GPU_Graph* g, GPU_Texture* dst, uint32_t mip, uint32_t r, uint32_t gg, uint32_t b, uint32_t a) {
    REC_GUARD(g); uint32_t u[4] = {r, gg, b, a}; record_clear(g, dst, mip, 1, nullptr, u, __func__);
}
GPU_API void GPU_OpClearDepthStencil(GPU_Graph* g, GPU_Texture* dst, uint32_t mip) {
    REC_GUARD(g);
    GPU_REQUIRE_V(dst && GPUX_GetFormatInfo(dst->format).depth_target, "GPU_OpClearDepthStencil: not a depth format");   // gpu_vulkan.c:2875
    float f[4] = {1.0f, 0, 0, 0}; record_clear(g, dst, mip, 2, f, nullptr, __func__);                                    // GPU_REVERSE_DEPTH false -> far = 1
}

// ------------------------------------------------------------------------------------------
// execution
// ------------------------------------------------------------------------------------------
static bool ensure_bordered(TextureImpl* t, hipStream_t st, int first_level = 0) {
    int W = (int)t->base.width, levels = (int)t->base.mip_level_count;
    if (first_level < 0) first_level = 0;
    if (first_level > levels - 1) first_level = levels - 1;
    TextureImpl::Derived& d = t->derived;
    if (d.bordered_valid && d.bordered_from <= first_level) return true;
    if (!d.bordered) {
        const size_t bytes = pbrk_bordered_pyramid_texels(W, levels) * 16;
        hipError_t e = hipMalloc(&d.bordered, bytes);
        if (e != hipSuccess) { gpu_fail("bordered twin allocation (%zu bytes) failed: %s", bytes, hipGetErrorString(e)); return false; }
    }
    // only the levels somebody samples get an apron (the precompute never touches level 0 of its source: 400 MB at 2048^2); a valid one is only extended
    int end = d.bordered_valid ? d.bordered_from : levels;
    int rc = pbrk_border_build_range(t->dev, d.bordered, W, levels, first_level, end, st);
    if (rc != PBRK_OK) { gpu_fail("border build failed (%d)", rc); return false; }
    d.bordered_valid = true; d.bordered_from = first_level;
    return true;
}

// {min, max} of the RGB values of level l (blocking: one reduction + an 8-byte read-back per level and content change)
static bool level_range(TextureImpl* t, int l, hipStream_t st, float* mn, float* mx) {
    const int levels = (int)t->base.mip_level_count;
    TextureImpl::Derived& d = t->derived;
    if (d.range_valid.empty()) { d.range_valid.assign((size_t)levels, 0); d.range_min.assign((size_t)levels, 0.0f); d.range_max.assign((size_t)levels, 0.0f); }
    if (!d.range_valid[(size_t)l]) {
        if (!d.range_dev && hipMalloc(&d.range_dev, 8) != hipSuccess) { d.range_dev = nullptr; return false; }
        const unsigned init[2] = {0x7F800000u, 0u};
        unsigned got[2] = {0, 0};
        HIP_OK(hipMemcpyAsync(d.range_dev, init, 8, hipMemcpyHostToDevice, st));
        const size_t n = mip_dim(t->base.width, (uint32_t)l);
        if (pbrk_level_minmax((const char*)t->dev + t->mip_offset[(size_t)l], 6 * n * n, d.range_dev, st) != PBRK_OK) return false;
        HIP_OK(hipMemcpyAsync(got, d.range_dev, 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        memcpy(&d.range_min[(size_t)l], &got[0], 4); memcpy(&d.range_max[(size_t)l], &got[1], 4);
        d.range_valid[(size_t)l] = 1;
    }
    *mn = d.range_min[(size_t)l]; *mx = d.range_max[(size_t)l];
    return true;
}
// Samples a prefilter dispatch keeps under GPUX_SetPrefilterTolerance(rel): the smallest prefix K of the weight table (weights fall
// with the sample index) with  tail(K) * max <= rel * head(K) * min.  Every tap is a convex combination of the level's texels, so a
// texel's dropped part is at most tail * max and what it keeps at least head * min: `rel` bounds the relative error of every
// texel and channel.  Sums in double, from the tail so that the small terms are not lost.
static int bounded_sample_count(const DeviceTable* tab, float mn, float mx, float rel) {
    const int n = tab->count;
    if (!(rel > 0.0f) || n < 2 || !(mn > 0.0f) || !(mx >= mn) || !isfinite(mx) || (int)tab->weights.size() != n) return n;
    double total = 0.0;
    for (int i = 0; i < n; ++i) total += (double)tab->weights[(size_t)i];
    double tail = 0.0;
    int K = n;
    for (int i = n - 1; i >= 1; --i) {                      // try K = i: drop samples i .. n-1
        const double t2 = tail + (double)tab->weights[(size_t)i];
        const double head = total - t2;
        if (!(t2 * (double)mx <= (double)rel * head * (double)mn)) break;
        tail = t2; K = i;
    }
    return K;
}

// cells twin of one level (needs a valid bordered twin); NULL when the level is too big to be worth it (n > 512)
static void* ensure_cells(TextureImpl* t, int level, hipStream_t st) {
    int W = (int)t->base.width, levels = (int)t->base.mip_level_count;
    TextureImpl::Derived& d = t->derived;
    if (d.cells_off.empty()) {
        int first = 0;
        while (first < levels && (W >> first) > 512) ++first;
        d.cells_first = first;
        size_t off = 0;
        for (int l = first; l < levels; ++l) { d.cells_off.push_back(off); int n = W >> l; if (n < 1) n = 1; off += pbrk_cells_bytes(n); }
        d.cells_off.push_back(off);
        d.cells_valid.assign(levels > first ? levels - first : 0, 0);
        if (off) {
            hipError_t e = hipMalloc(&d.cells, off);
            if (e != hipSuccess) { d.cells = nullptr; gpu_fail("cells twin allocation (%zu bytes) failed: %s", off, hipGetErrorString(e)); }
        }
    }
    if (!d.cells || level < d.cells_first || level >= levels) return nullptr;
    int li = level - d.cells_first;
    void* c = (char*)d.cells + d.cells_off[li];
    if (d.cells_valid[li]) return c;
    int n = W >> level; if (n < 1) n = 1;
    const void* src = (const char*)d.bordered + pbrk_bordered_level_offset(W, level) * 16;
    if (pbrk_cells_build(src, n, c, st) != PBRK_OK) return nullptr;
    d.cells_valid[li] = 1;
    return c;
}
static bool cells_ready(const TextureImpl* t, int level) {
    const int li = level - t->derived.cells_first;
    return t->derived.cells && li >= 0 && li < (int)t->derived.cells_valid.size() && t->derived.cells_valid[li];
}

static bool apron_ready(const TextureImpl* t, int first_level) { return t->derived.bordered_valid && t->derived.bordered_from <= first_level; }
static float reference_roughness(int mip) {                      // gen_prefiltered_env_map.glsl:117 + SURVEY 8d extension
    static const float tab[5] = {0.0f, 0.03f, 0.15f, 0.4f, 0.6f};
    if (mip < 5) return tab[mip < 0 ? 0 : mip];
    float r = 0.6f + 0.08f * (float)(mip - 4);
    return r > 1.0f ? 1.0f : r;
}

static hipEvent_t next_sync_event(GPU_Graph* g) {
    if (g->sync_used == g->sync_ev.size()) { hipEvent_t e; HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); g->sync_ev.push_back(e); }
    return g->sync_ev[g->sync_used++];
}

// Lazily built twins (apron, cells) enqueued on a side stream must be visible to the launches that follow on every other stream.
static void publish_side_work(GPU_Graph* g) {
    if (g->cur == g->stream) return;
    hipEvent_t e = next_sync_event(g);
    HIP_OK(hipEventRecord(e, g->cur));
    HIP_OK(hipStreamWaitEvent(g->stream, e, 0));
    for (hipStream_t s : g->side) if (s != g->cur) HIP_OK(hipStreamWaitEvent(s, e, 0));
}

// ---- one function per kernel family; exec_op at the end of the section picks one by the op's kind and kernel ----
static void exec_sweep(GPU_Graph* g, Op& op, size_t& ev_used) {
    TextureImpl* it = named_slot(op.set, "IMG0")->tex;
    int32_t dir; memcpy(&dir, op.push, 4);
    timed(g, dir == 0 ? "K7.sweep_x" : (dir == 1 ? "K7.sweep_y" : "K7.sweep_z"), ev_used, [&] {
        int rc = pbrk_lightgrid_sweep(it->dev, (int)it->base.width, (int)it->base.height, (int)it->base.depth, dir,
                                      (int)op.row0, (int)op.row1, (int)op.face0, (int)op.face1, g->cur);
        if (rc != PBRK_OK) gpu_fail("K7 launch failed (%d)", rc);
    });
}

// The push constants of a precompute dispatch: a whole GPUX_IBLConstants block (true), or the reference's 4-byte `int mip_level`
static bool ibl_constants(const Op& op, GPUX_IBLConstants& c) {
    c = {0, 0.0f, 0.0f, 0};
    if (op.push_size == sizeof(GPUX_IBLConstants)) { memcpy(&c, op.push, sizeof c); return true; }
    if (op.push_size >= 4) memcpy(&c.mip_level, op.push, 4);
    return false;
}

static void exec_brdf_lut(GPU_Graph* g, Op& op, size_t& ev_used) {
    Slot* out = named_slot(op.set, "OUTPUT");
    TextureImpl* ot = out->tex;
    uint32_t size = mip_dim(ot->base.width, out->mip);
    void* out_ptr = (char*)ot->dev + ot->mip_offset[out->mip];
    GPUX_IBLConstants c;
    const bool explicit_c = ibl_constants(op, c);
    int n = (explicit_c && c.sample_count > 0) ? c.sample_count : 4096;
    DeviceTable* ang = get_table(2, n, 0.0f, 0);
    DeviceTable* vcs = get_table(3, (int)size, 0.0f, 0);
    if (!ang || !vcs) return;
    int fmt = ot->base.format == GPU_Format_RG16F ? PBRK_FMT_RG16F : (ot->base.format == GPU_Format_RG32F ? PBRK_FMT_RG32F : PBRK_FMT_RGBA32F);
    timed(g, "K1.brdf_lut", ev_used, [&] {
        int rc = pbrk_brdf_lut(out_ptr, fmt, (int)size, n, ang->dev, vcs->dev, (int)op.row0, (int)op.row1, g->cur);
        if (rc != PBRK_OK) gpu_fail("K1 launch failed (%d)", rc);
    });
}

// What an irradiance (K3) or prefilter (K4a: the copy of mip 0, K4b: Monte Carlo) dispatch asks for, decoded once from its push
// constants: exec_ibl_filter launches from it, dispatch_samples_per_texel sizes the dispatch with it.
struct IblPlan {
    bool ok = true;                  // false: nothing can be launched (bad_roughness, or the table could not be made)
    bool bad_roughness = false;      // a Monte-Carlo mip with roughness <= 0: only exec_ibl_filter reports it
    bool copy = false;               // K4a
    int mip = 0;                     // the prefilter's branch and output mip (c.mip_level)
    float lod = 0.0f;                // source LOD
    int n = 0;                       // samples asked for (the copy: 0)
    float rough = 0.0f, divisor = 1.0f;
    int table_kind = -1;             // get_table kind (0: prefilter, 1: irradiance; -1: the copy has none)
    DeviceTable* tab = nullptr;      // that table
    char name[96];                   // its GPUX_GraphTimedOpName
};
static IblPlan plan_ibl(const Op& op) {
    IblPlan p;
    GPUX_IBLConstants c;
    const bool explicit_c = ibl_constants(op, c);
    p.mip = c.mip_level;
    if (op.cpipe->kernel == Kernel_Irradiance) {
        p.lod = explicit_c ? c.src_lod : 6.0f;                   // gen_irradiance_map.glsl:94
        p.n = (explicit_c && c.sample_count > 0) ? c.sample_count : 1024;
        p.divisor = (float)p.n; p.table_kind = 1;
        snprintf(p.name, sizeof p.name, "K3.irradiance");
    } else if (p.mip == 0) {
        p.copy = true; p.lod = explicit_c ? c.src_lod : 1.0f;
        snprintf(p.name, sizeof p.name, "K4a.prefilter_copy.mip%d", p.mip);
    } else {
        p.lod = explicit_c ? c.src_lod : 3.0f + (float)p.mip;
        p.n = (explicit_c && c.sample_count > 0) ? c.sample_count : 8192;
        p.rough = explicit_c ? c.roughness : reference_roughness(p.mip);
        p.divisor = 3.14159265358979323846f; p.table_kind = 0;
        snprintf(p.name, sizeof p.name, "K4b.prefilter_mc.mip%d", p.mip);
        if (!(p.rough > 0.0f)) { p.bad_roughness = true; p.ok = false; return p; }
    }
    if (p.table_kind >= 0) {
        p.tab = get_table(p.table_kind, p.n, p.rough, 0);        // cached; only entries with non-zero weight are kept
        p.ok = p.tab != nullptr;
    }
    return p;
}

// The level of `et` a launchable plan samples; -1 for a fractional LOD inside the chain, which the precompute kernels do not take
static int ibl_source_level(const TextureImpl* et, const IblPlan& p) {
    const int levels = (int)et->base.mip_level_count;
    int l = (int)floorf(p.lod);
    if (l < 0) l = 0;
    if (l > levels - 1) l = levels - 1;                     // sampler clamps LOD to the chain
    return ((float)l != p.lod && p.lod < (float)(levels - 1)) ? -1 : l;
}

// The twins a precompute dispatch samples -- the apron from level l on and, unless it is the copy, the cells of level l -- built on
// g->cur where they are missing, and published.  False: the apron could not be built (reported).
static bool ensure_ibl_twins(GPU_Graph* g, TextureImpl* et, int l, bool want_cells, size_t& ev_used) {
    hipStream_t st = g->cur;
    if (!apron_ready(et, l)) {
        timed(g, "apron.env", ev_used, [&] { ensure_bordered(et, st, l); });
        if (!apron_ready(et, l)) return false;
        publish_side_work(g);
    }
    if (want_cells && !cells_ready(et, l)) {
        const void* built = nullptr;
        timed(g, "cells.env", ev_used, [&] { built = ensure_cells(et, l, st); });
        if (built) publish_side_work(g);                    // a level too big for a cells twin enqueues nothing
    }
    return true;
}

static void exec_ibl_filter(GPU_Graph* g, Op& op, size_t& ev_used) {
    hipStream_t st = g->cur;
    Slot* out = named_slot(op.set, "OUTPUT");
    TextureImpl* ot = out->tex;
    uint32_t size = mip_dim(ot->base.width, out->mip);
    void* out_ptr = (char*)ot->dev + ot->mip_offset[out->mip];
    TextureImpl* et = named_slot(op.set, "TEX_ENV_CUBE")->tex;
    int W = (int)et->base.width;
    const IblPlan p = plan_ibl(op);
    if (p.bad_roughness) { gpu_fail("prefilter: roughness must be > 0 for Monte-Carlo mips (got %g)", p.rough); return; }
    if (!p.ok) return;
    const bool mc_prefilter = op.cpipe->kernel == Kernel_Prefilter && !p.copy;
    const int l = ibl_source_level(et, p);
    if (l < 0) { gpu_fail("%s: fractional source LOD %g is not supported by the precompute kernels", p.name, p.lod); return; }
    if (!ensure_ibl_twins(g, et, l, !p.copy, ev_used)) return;
    int n_src = W >> l; if (n_src < 1) n_src = 1;
    const void* src = (const char*)et->derived.bordered + pbrk_bordered_level_offset(W, l) * 16;
    const void* cells = p.copy ? nullptr : ensure_cells(et, l, st);          // built by now: the pointer (NULL: the level has no cells twin)
    int n_keep = p.tab ? p.tab->count : 0;
    if (mc_prefilter && G.prefilter_tol > 0.0f) {            // opt-in: tolerance-budgeted sample cut (gpux.h)
        float mn = 0.0f, mx = 0.0f;
        if (level_range(et, l, st, &mn, &mx)) n_keep = bounded_sample_count(p.tab, mn, mx, G.prefilter_tol);
    }
    if (mc_prefilter && p.mip >= 0 && p.mip < 32) G.kept_samples[p.mip] = n_keep;
    const float alpha = p.table_kind == 0 ? p.tab->alpha : 0.0f;
    timed(g, p.name, ev_used, [&] {
        int rc = p.copy ? pbrk_prefilter_copy(src, n_src, out_ptr, (int)size, (int)op.face0, (int)op.face1, (int)op.row0, (int)op.row1, st)
                        : pbrk_mc_filter(src, cells, n_src, p.tab->dev, n_keep, p.divisor, alpha, out_ptr, (int)size,
                                         (int)op.face0, (int)op.face1, (int)op.row0, (int)op.row1, st);
        if (rc != PBRK_OK) gpu_fail("%s launch failed (%d)", p.name, rc);
    });
}

// sample evaluations per output texel of a precompute dispatch
static double dispatch_samples_per_texel(const Op& op) {
    const IblPlan p = plan_ibl(op);
    if (op.cpipe->kernel == Kernel_Irradiance) return p.n;
    if (p.copy) return 4.0;                                                 // the copy level: one bilinear fetch, HBM-bound
    return p.tab ? (double)p.tab->count : (double)p.n;
}

// Builds a precompute dispatch's twins ahead of its launch (on g->cur); a dispatch that cannot be launched is left to exec_ibl_filter.
static void prepare_ibl_twins(GPU_Graph* g, const Op& op, size_t& ev_used) {
    TextureImpl* et = named_slot(op.set, "TEX_ENV_CUBE")->tex;
    const IblPlan p = plan_ibl(op);
    const int l = p.ok ? ibl_source_level(et, p) : -1;
    if (l >= 0) ensure_ibl_twins(g, et, l, !p.copy, ev_used);
}

static void exec_bloom(GPU_Graph* g, Op& op, size_t& ev_used) {
    GPU_RenderPass* rp = op.pass;
    TextureImpl* target = (TextureImpl*)rp->targets[0].texture;
    TextureImpl* in = named_slot(op.set, "TEX0")->tex;
    PbrkBloomArgs a;
    a.src.data = (char*)in->dev + in->mip_offset[op.mip]; a.src.format = PBRK_FMT_RGBA16F;
    a.src.width = (int)mip_dim(in->base.width, op.mip); a.src.height = (int)mip_dim(in->base.height, op.mip);
    a.dst = (char*)target->dev + target->mip_offset[op.mip2];
    a.dst_width = (int)rp->desc.width; a.dst_height = (int)rp->desc.height;
    int32_t lvl; memcpy(&lvl, op.push, 4); a.dst_mip_level = lvl;
    a.upsample = op.gpipe->kernel == Kernel_BloomUp; a.blend_additive = op.gpipe->blend_additive;
    a.blend_src = op.blend_tex ? (const void*)((const char*)op.blend_tex->dev + op.blend_tex->mip_offset[op.blend_mip]) : nullptr;
    a.y0 = (int)op.row0; a.y1 = (int)op.row1;
    timed(g, a.upsample ? "K11.bloom_upsample" : "K10.bloom_downsample", ev_used, [&] {
        int rc = pbrk_bloom_pass(&a, g->cur);
        if (rc != PBRK_OK) gpu_fail("bloom launch failed (%d)", rc);
    });
}

static void exec_taa(GPU_Graph* g, Op& op, size_t& ev_used) {
    GPU_DescriptorSet* s = op.set;
    GPU_RenderPass* rp = op.pass;
    TextureImpl* target = (TextureImpl*)rp->targets[0].texture;
    PbrkTaaArgs a;
    a.lighting_result = tex2d(named_slot(s, "LIGHTING_RESULT")->tex, PBRK_FMT_RGBA16F);
    a.gbuffer_depth = tex2d(named_slot(s, "GBUFFER_DEPTH")->tex, PBRK_FMT_R32F);
    a.gbuffer_velocity = tex2d(named_slot(s, "GBUFFER_VELOCITY")->tex, PBRK_FMT_RG16F);
    a.gbuffer_velocity_prev = tex2d(named_slot(s, "GBUFFER_VELOCITY_PREV")->tex, PBRK_FMT_RG16F);
    a.prev_frame_result = tex2d(named_slot(s, "PREV_FRAME_RESULT")->tex, PBRK_FMT_RGBA16F);
    a.out = target->dev; a.out_format = out_fmt(target->base.format);
    a.width = (int)rp->desc.width; a.height = (int)rp->desc.height; a.y0 = (int)op.row0; a.y1 = (int)op.row1;
    timed(g, "K8.taa_resolve", ev_used, [&] {
        int rc = pbrk_taa_resolve(&a, g->cur);
        if (rc != PBRK_OK) gpu_fail("K8 launch failed (%d)", rc);
    });
}

static void exec_final(GPU_Graph* g, Op& op, size_t& ev_used) {
    GPU_RenderPass* rp = op.pass;
    TextureImpl* target = (TextureImpl*)rp->targets[0].texture;
    PbrkFinalArgs a;
    a.src = tex2d(named_slot(op.set, "TEX0")->tex, PBRK_FMT_RGBA16F);
    a.out = target->dev; a.out_format = out_fmt(target->base.format);
    a.width = (int)rp->desc.width; a.height = (int)rp->desc.height; a.y0 = (int)op.row0; a.y1 = (int)op.row1;
    timed(g, "K9.final_post_process", ev_used, [&] {
        int rc = pbrk_final_post_process(&a, g->cur);
        if (rc != PBRK_OK) gpu_fail("K9 launch failed (%d)", rc);
    });
}

// K16 over the rows of a lighting op whose Globals (`globals`: the 552 bytes exec_shade has just read) set visualize_lightgrid
static void exec_gridview(GPU_Graph* g, Op& op, size_t& ev_used, const float* globals) {
    GPU_RenderPass* rp = op.pass;
    TextureImpl* target = (TextureImpl*)rp->targets[0].texture;
    Slot* gs = named_slot(op.set, "LIGHTGRID");
    TextureImpl* grid = gs ? gs->tex : nullptr;
    GPU_REQUIRE_V(grid && grid->base.format == GPU_Format_RGBA16F && grid->base.layer_count == 1 && grid->base.depth >= 2 &&
                  grid->base.width == grid->base.depth && grid->base.height == grid->base.depth && grid->base.depth <= 1024,
                  "lighting pass: visualize_lightgrid is set, but \"LIGHTGRID\" is not bound to a cubic RGBA16F 3-D texture (render.cpp:678); nothing drawn");
    PbrkGridViewArgs v;
    v.width = (int)rp->desc.width; v.height = (int)rp->desc.height;
    v.x0 = 0; v.x1 = v.width; v.y0 = (int)op.row0; v.y1 = (int)op.row1;
    v.lightgrid = grid->dev; v.lightgrid_size = (int)grid->base.width;
    v.out = target->dev; v.out_format = target->base.format == GPU_Format_RGBA16F ? PBRK_FMT_RGBA16F : PBRK_FMT_RGBA32F;
    memcpy(v.globals, globals, sizeof v.globals);
    g->launch_sig.push_back(16);
    timed(g, "K16.gridview", ev_used, [&] {
        int rc = pbrk_lightgrid_view(&v, g->cur);
        if (rc != PBRK_OK) gpu_fail("K16 launch failed (%d)", rc);
    });
}

// The sampler twins that the lighting op (K5) reads and that are built lazily, in the order exec_shade builds them: the apron of the
// prefiltered cube from level 0 and the cells of its levels of size <= 512; under GPUX_Shade_IBL the apron and the level-0 cells of
// the irradiance cube and the cells of the BRDF LUT.  exec_shade builds what is missing of them, op_replayable asks whether anything
// is, graph_replayable takes the sampled maps from them.
enum TwinKind { Twin_Apron, Twin_SmallCells /* of every level of size <= 512 */, Twin_Cells0 /* of level 0 */, Twin_LutCells };
struct ShadeTwin { TextureImpl* tex; TwinKind kind; const char* timed_name; /* of its build; NULL: not timed */ };
static int shade_twins(GPU_DescriptorSet* s, int shade_flags, ShadeTwin tw[5], bool sh9 = false /* the op shades from SH9 coefficients: no irradiance twin */) {
    auto tex = [&](const char* name) { Slot* sl = named_slot(s, name); return sl ? sl->tex : nullptr; };
    int n = 0;
    if (TextureImpl* pre = tex("PREFILTERED_ENV_MAP")) { tw[n++] = {pre, Twin_Apron, "apron.prefiltered"}; tw[n++] = {pre, Twin_SmallCells, "cells.prefiltered"}; }
    if (!(shade_flags & GPUX_Shade_IBL)) return n;
    if (!sh9) if (TextureImpl* irr = tex("TEX_IRRADIANCE_MAP")) { tw[n++] = {irr, Twin_Apron, "apron.irradiance"}; tw[n++] = {irr, Twin_Cells0, nullptr}; }
    if (TextureImpl* lut = tex("BRDF_INTEGRATION_MAP")) tw[n++] = {lut, Twin_LutCells, nullptr};
    return n;
}
static bool shade_twin_ready(const ShadeTwin& tw) {
    TextureImpl* t = tw.tex;
    switch (tw.kind) {
    case Twin_Apron: return apron_ready(t, 0);
    case Twin_SmallCells:
        for (int l = 0; l < (int)t->base.mip_level_count; ++l) if (((int)t->base.width >> l) <= 512 && !cells_ready(t, l)) return false;
        return true;
    case Twin_Cells0: return cells_ready(t, 0);
    case Twin_LutCells: return t->derived.lut_cells_valid;
    }
    return false;
}
// Builds a missing twin on the graph's main stream.  False: the op cannot be launched (its apron failed; K5 does without cells).
static bool build_shade_twin(GPU_Graph* g, const ShadeTwin& tw, size_t& ev_used) {
    TextureImpl* t = tw.tex;
    switch (tw.kind) {
    case Twin_Apron:
        timed(g, tw.timed_name, ev_used, [&] { ensure_bordered(t, g->stream); });
        return apron_ready(t, 0);
    case Twin_SmallCells:
        timed(g, tw.timed_name, ev_used, [&] { for (int l = 0; l < (int)t->base.mip_level_count; ++l) if (((int)t->base.width >> l) <= 512) ensure_cells(t, l, g->stream); });
        return true;
    case Twin_Cells0: ensure_cells(t, 0, g->stream); return true;
    case Twin_LutCells: {
        const int n = (int)t->base.width;
        TextureImpl::Derived& d = t->derived;
        if (!d.lut_cells && hipMalloc(&d.lut_cells, (size_t)(n + 1) * (n + 1) * 16) != hipSuccess) d.lut_cells = nullptr;
        if (d.lut_cells && pbrk_lut_cells_build(t->dev, n, d.lut_cells, g->stream) == PBRK_OK) d.lut_cells_valid = true;
        return true;
    }
    }
    return false;
}
static void* cells_of(TextureImpl* t, int level) { return cells_ready(t, level) ? (char*)t->derived.cells + t->derived.cells_off[(size_t)(level - t->derived.cells_first)] : nullptr; }

static void exec_shade(GPU_Graph* g, Op& op, size_t& ev_used) {
    GPU_DescriptorSet* s = op.set;
    GPU_RenderPass* rp = op.pass;
    TextureImpl* target = (TextureImpl*)rp->targets[0].texture;
    PbrkShadeArgs a;
    memset(&a, 0, sizeof a);
    a.width = (int)rp->desc.width; a.height = (int)rp->desc.height;
    a.x0 = 0; a.x1 = a.width; a.y0 = (int)op.row0; a.y1 = (int)op.row1;
    // Globals first: visualize_lightgrid (word 137, main.cpp:79 / render.cpp:990) replaces the whole shading of every pixel with the
    // light-grid ray march (lighting_pass.glsl:463-491) -- K16 over the same rows, none of K5's aprons / twins, whatever the flags
    read_globals(named_slot(s, "GLOBALS")->buf, 0, a.globals, 552);
    uint32_t visualize; memcpy(&visualize, &a.globals[137], 4);
    if (visualize != 0) { exec_gridview(g, op, ev_used, a.globals); return; }
    g->launch_sig.push_back(5);
    a.base_color = named_slot(s, "GBUFFER_BASE_COLOR")->tex->dev;
    a.normal = named_slot(s, "GBUFFER_NORMAL")->tex->dev;
    a.orm = named_slot(s, "GBUFFER_ORM")->tex->dev;
    a.emissive = named_slot(s, "GBUFFER_EMISSIVE")->tex->dev;
    a.depth = named_slot(s, "GBUFFER_DEPTH")->tex->dev;
    ShadeTwin tw[5];
    const bool sh9 = op.buf != nullptr;                                      // as recorded (record_shade)
    const int n_tw = shade_twins(s, op.gpipe->shade_flags, tw, sh9);
    for (int i = 0; i < n_tw; ++i) if (!shade_twin_ready(tw[i]) && !build_shade_twin(g, tw[i], ev_used)) return;
    TextureImpl* pre = named_slot(s, "PREFILTERED_ENV_MAP")->tex;
    a.prefiltered_bordered = pre->derived.bordered; a.prefiltered_size = (int)pre->base.width; a.prefiltered_levels = (int)pre->base.mip_level_count;
    a.prefiltered_cells = pre->derived.cells; a.prefiltered_cells_first = pre->derived.cells_first;
    a.flags = 0;
    if (op.gpipe->shade_flags & GPUX_Shade_IBL) {
        a.flags |= PBRK_SHADE_IBL;
        if (sh9) {
            a.flags |= PBRK_SHADE_SH9;
            a.sh9_coef = (const double*)((const char*)op.buf->dev + op.off_a);
        } else {
            TextureImpl* irr = named_slot(s, "TEX_IRRADIANCE_MAP")->tex;
            a.irradiance_bordered = irr->derived.bordered; a.irradiance_size = (int)irr->base.width;
            a.irradiance_cells = cells_of(irr, 0);
        }
        TextureImpl* lut = named_slot(s, "BRDF_INTEGRATION_MAP")->tex;
        a.lut = lut->dev; a.lut_size = (int)lut->base.width;
        a.lut_cells = lut->derived.lut_cells_valid ? lut->derived.lut_cells : nullptr;
    }
    if (op.gpipe->shade_flags & GPUX_Shade_VoxelGI) {
        a.flags |= PBRK_SHADE_GI;
        TextureImpl* grid = named_slot(s, "LIGHTGRID")->tex;
        a.lightgrid = grid->dev; a.lightgrid_size = (int)grid->base.width;
        TextureImpl* prev = named_slot(s, "PREV_FRAME_RESULT")->tex;
        a.prev_frame_levels = (int)(prev->base.mip_level_count < 8 ? prev->base.mip_level_count : 8);
        a.prev_frame_w = (int)prev->base.width; a.prev_frame_h = (int)prev->base.height;
        for (int l = 0; l < a.prev_frame_levels; ++l) a.prev_frame[l] = (char*)prev->dev + prev->mip_offset[l];
        if (!(op.gpipe->shade_flags & GPUX_Shade_IBL)) {                   // the LUT fetch of :681 feeds the GI specular term too
            TextureImpl* lut = named_slot(s, "BRDF_INTEGRATION_MAP")->tex;
            a.lut = lut->dev; a.lut_size = (int)lut->base.width;
        }
    }
    if (op.gpipe->shade_flags & GPUX_Shade_LightShafts) a.flags |= PBRK_SHADE_SHAFTS;
    if (op.gpipe->shade_flags & GPUX_Shade_SunShadows) {
        TextureImpl* sun = named_slot(s, "SUN_DEPTH_MAP")->tex;
        a.flags |= PBRK_SHADE_SHADOWS;
        a.sun_depth = sun->dev; a.sun_depth_w = (int)sun->base.width; a.sun_depth_h = (int)sun->base.height;
    }
    a.out = target->dev;
    a.out_format = target->base.format == GPU_Format_RGBA16F ? PBRK_FMT_RGBA16F : PBRK_FMT_RGBA32F;
    timed(g, "K5.shade", ev_used, [&] {
        int rc = pbrk_shade(&a, g->cur);
        if (rc != PBRK_OK) gpu_fail("K5 launch failed (%d)", rc);
    });
}

static void exec_mipgen(GPU_Graph* g, Op& op, size_t& ev_used) {
    timed(g, op.name, ev_used, [&] {
        int rc = is_rgba8_pow2(op.tex) ? pbrk_mip_chain_rgba8(op.tex->dev, (int)op.tex->base.width, (int)op.tex->base.height, (int)op.tex->base.mip_level_count, g->cur)
                                       : pbrk_mip_chain(op.tex->dev, (int)op.tex->base.width, (int)op.tex->base.mip_level_count, g->cur);
        if (rc != PBRK_OK) gpu_fail("K2 launch failed (%d)", rc);
    });
}

// K17: two launches (partials, then their sum in index order) resp. one; no read-back, nothing allocated
static void exec_sh9(GPU_Graph* g, Op& op, size_t& ev_used) {
    const int n = (int)mip_dim(op.tex->base.width, op.mip);
    void* level = (char*)op.tex->dev + op.tex->mip_offset[op.mip];
    double* coef = (double*)((char*)op.buf->dev + op.off_b);
    timed(g, op.name, ev_used, [&] {
        int rc = op.kind == Op_ProjectSH9
                     ? pbrk_sh9_project(level, n, (int)op.face0, (int)op.face1, (int)op.row0, (int)op.row1, g->sh_scratch, coef, g->cur)
                     : pbrk_sh9_irradiance(coef, level, n, (int)op.face0, (int)op.face1, (int)op.row0, (int)op.row1, g->cur);
        if (rc != PBRK_OK) gpu_fail("%s launch failed (%d)", op.name.c_str(), rc);
    });
}

// K18, either quality: one launch; nothing read back, nothing allocated
static void exec_bc6h(GPU_Graph* g, Op& op, size_t& ev_used) {
    const GPU_Texture& t = op.tex->base;
    const void* level = (const char*)op.tex->dev + op.tex->mip_offset[op.mip];
    const auto encode = op.quality == GPUX_BC6H_TwoRegions ? pbrk_bc6h_encode2 : pbrk_bc6h_encode;
    timed(g, op.name, ev_used, [&] {
        int rc = encode(level, bc6h_source_format(t.format), (int)mip_dim(t.width, op.mip), (int)mip_dim(t.height, op.mip), (int)t.layer_count,
                        (char*)op.buf->dev + op.off_b, g->cur);
        if (rc != PBRK_OK) gpu_fail("%s launch failed (%d)", op.name.c_str(), rc);
    });
}

// K19: one launch
static void exec_bc6h_decode(GPU_Graph* g, Op& op, size_t& ev_used) {
    const GPU_Texture& t = op.tex->base;
    void* level = (char*)op.tex->dev + op.tex->mip_offset[op.mip];
    timed(g, op.name, ev_used, [&] {
        int rc = pbrk_bc6h_decode((const char*)op.buf->dev + op.off_a, (int)mip_dim(t.width, op.mip), (int)mip_dim(t.height, op.mip), (int)t.layer_count, level,
                                  bc6h_source_format(t.format), g->cur);
        if (rc != PBRK_OK) gpu_fail("%s launch failed (%d)", op.name.c_str(), rc);
    });
}

// K20: the apron of the cube from the source level on where it is missing (its own timed entry), then one launch; nothing allocated
static void exec_panorama(GPU_Graph* g, Op& op, size_t& ev_used) {
    TextureImpl* cube = op.tex;
    const GPU_Texture& d = op.tex2->base;
    const int W = (int)cube->base.width;
    if (!apron_ready(cube, (int)op.mip)) {
        timed(g, "apron.panorama", ev_used, [&] { ensure_bordered(cube, g->cur, (int)op.mip); });
        if (!apron_ready(cube, (int)op.mip)) return;
    }
    const void* level = (const char*)cube->derived.bordered + pbrk_bordered_level_offset(W, (int)op.mip) * 16;
    void* out = (char*)op.tex2->dev + op.tex2->mip_offset[op.mip2];
    timed(g, op.name, ev_used, [&] {
        int rc = pbrk_cube_to_panorama(level, (int)mip_dim(cube->base.width, op.mip), op.pano_table, out, bc6h_source_format(d.format),
                                       (int)mip_dim(d.width, op.mip2), (int)mip_dim(d.height, op.mip2), g->cur);
        if (rc != PBRK_OK) gpu_fail("%s launch failed (%d)", op.name.c_str(), rc);
    });
}

// K21: the whole apron of the source where it is missing (its own timed entry: a sample may name any level), then one launch
static void exec_prefilter_ggx(GPU_Graph* g, Op& op, size_t& ev_used) {
    TextureImpl* env = op.tex;
    if (!apron_ready(env, 0)) {
        timed(g, "apron.prefilter_ggx", ev_used, [&] { ensure_bordered(env, g->cur, 0); });
        if (!apron_ready(env, 0)) return;
    }
    void* out = (char*)op.tex2->dev + op.tex2->mip_offset[op.mip2];
    timed(g, op.name, ev_used, [&] {
        int rc = pbrk_prefilter_ggx(env->derived.bordered, op.ggx_table, (int)op.ggx_kept, op.ggx_wsum, out, (int)mip_dim(op.tex2->base.width, op.mip2),
                                    (int)op.face0, (int)op.face1, (int)op.row0, (int)op.row1, g->cur);
        if (rc != PBRK_OK) gpu_fail("%s launch failed (%d)", op.name.c_str(), rc);
    });
}

// K22: one launch on level 0; the table exists since recording, nothing is allocated
static void exec_brdf_lut_ggx(GPU_Graph* g, Op& op, size_t& ev_used) {
    const GPU_Texture& t = op.tex->base;
    const int fmt = t.format == GPU_Format_RG16F ? PBRK_FMT_RG16F : (t.format == GPU_Format_RG32F ? PBRK_FMT_RG32F : PBRK_FMT_RGBA32F);
    timed(g, op.name, ev_used, [&] {
        int rc = pbrk_brdf_lut_ggx(op.tex->dev, fmt, (int)t.width, (int)t.height, (int)op.lut_samples, (int)op.lut_visibility, op.lut_table,
                                   (int)op.row0, (int)op.row1, g->cur);
        if (rc != PBRK_OK) gpu_fail("%s launch failed (%d)", op.name.c_str(), rc);
    });
}

static void exec_blit(GPU_Graph* g, Op& op, size_t& ev_used) {
    hipStream_t st = g->cur;
    if (op.folded) return;                                                 // its consumer reads the source (fold_blits)
    uint32_t nsw = mip_dim(op.tex->base.width, op.mip), nsh = mip_dim(op.tex->base.height, op.mip);
    uint32_t ndw = mip_dim(op.tex2->base.width, op.mip2), ndh = mip_dim(op.tex2->base.height, op.mip2);
    // op.size: a 1:1 copy of one layer of that many bytes; 0: a scaled blit between RGBA32F layers
    size_t layer_bytes_s = op.size ? op.size : (size_t)nsw * nsh * 16, layer_bytes_d = op.size ? op.size : (size_t)ndw * ndh * 16;
    const void* src = (const char*)op.tex->dev + op.tex->mip_offset[op.mip] + layer_bytes_s * op.layer0;
    void* dst = (char*)op.tex2->dev + op.tex2->mip_offset[op.mip2] + layer_bytes_d * op.layer2;
    timed(g, op.name, ev_used, [&] {
        if (op.size) { HIP_OK(hipMemcpyAsync(dst, src, op.size, hipMemcpyDeviceToDevice, st)); return; }
        int rc = (nsw == nsh && ndw == ndh && nsw == 2 * ndw) ? pbrk_box_downsample(src, (int)nsw, dst, 1, st)
                                                              : pbrk_blit_linear(src, (int)nsw, (int)nsh, dst, (int)ndw, (int)ndh, 1, st);
        if (rc != PBRK_OK) gpu_fail("blit launch failed (%d)", rc);
    });
}

// the four memcpy ops
static void exec_copy(GPU_Graph* g, Op& op, size_t& ev_used) {
    hipStream_t st = g->cur;
    switch (op.kind) {
    case Op_CopyB2B:
        timed(g, op.name, ev_used, [&] { HIP_OK(hipMemcpyAsync((char*)op.buf2->dev + op.off_b, (const char*)op.buf->dev + op.off_a, op.size, hipMemcpyDefault, st)); });
        return;
    case Op_CopyB2T: {
        uint64_t per_layer = GPUX_TextureMipBytes(&op.tex->base, op.mip) / op.tex->base.layer_count;
        timed(g, op.name, ev_used, [&] {
            HIP_OK(hipMemcpyAsync((char*)op.tex->dev + op.tex->mip_offset[op.mip] + per_layer * op.layer0, (const char*)op.buf->dev + op.off_a,
                                  per_layer * op.layer_count, hipMemcpyDefault, st));
        });
        if (op.tex->decoded) {                                                 // K15: the level that was written, and only it
            timed(g, "K15.bc_decode", ev_used, [&] {
                int rc = decode_bc_level(op.tex, op.mip, st);
                if (rc != PBRK_OK) gpu_fail("K15 launch failed (%d)", rc);
            });
        }
        return;
    }
    case Op_CopyDecodedT2B:
        timed(g, op.name, ev_used, [&] {
            HIP_OK(hipMemcpyAsync((char*)op.buf->dev + op.off_b, (const char*)op.tex->decoded + op.tex->decoded_offset[op.mip], op.size, hipMemcpyDefault, st));
        });
        return;
    case Op_CopyT2B:
        timed(g, op.name, ev_used, [&] {
            HIP_OK(hipMemcpyAsync((char*)op.buf->dev + op.off_b, (const char*)op.tex->dev + op.tex->mip_offset[op.mip],
                                  GPUX_TextureMipBytes(&op.tex->base, op.mip), hipMemcpyDefault, st));
        });
        return;
    default: return;
    }
}

// a clear is ONE fill launch for these texel sizes, at every alignment (k_cube.hip); the staged form of the others synchronises
static bool fill_texel_ok(uint32_t tb) { return tb == 1 || tb == 2 || tb == 4 || tb == 8 || tb == 16; }

static void exec_clear(GPU_Graph* g, Op& op, size_t& ev_used) {
    (void)ev_used;                                                             // clears are not timed
    hipStream_t st = g->cur;
    TextureImpl* t = op.tex;
    // Levels are back to back in the allocation ([mip][layer][y][x], tight), so GPU_MIP_LEVEL_ALL is ONE fill of the whole
    // texture instead of one per level: the reference clears bloom_upscale_rt this way every frame (render.cpp:1156; 11 levels at
    // 1080p = 11 fill kernels of ~5 us each in rocprofv3's trace, a quarter of the post-process tail, before round 3).
    const bool whole = op.mip == GPU_MIP_LEVEL_ALL;
    const uint32_t m = whole ? 0 : op.mip;
    size_t bytes = whole ? t->bytes : (size_t)GPUX_TextureMipBytes(&t->base, m);
    void* p = (char*)t->dev + t->mip_offset[m];
    if (whole && op.skip_level0) { p = (char*)t->dev + t->mip_offset[1]; bytes = t->bytes - t->mip_offset[1]; }   // fold_blits
    // build one texel pattern on the host and replicate it (clears are rare: upload a staging row)
    uint32_t tb = t->texel_bytes;
    std::vector<uint8_t> texel(tb, 0);
    if (op.clear_mode == 2 || t->base.format == GPU_Format_R32F) { memcpy(texel.data(), &op.clear[0], 4 < tb ? 4 : tb); }
    else if (op.clear_mode == 1) { for (uint32_t k = 0; k * 4 < tb && k < 4; ++k) memcpy(texel.data() + 4 * k, &op.cleari[k], 4); }
    else if (t->base.format == GPU_Format_RGBA32F || t->base.format == GPU_Format_RG32F) { memcpy(texel.data(), op.clear, tb); }
    else if (t->base.format == GPU_Format_RGBA8UN || t->base.format == GPU_Format_BGRA8UN) {
        int order[4] = {0, 1, 2, 3};
        if (t->base.format == GPU_Format_BGRA8UN) { order[0] = 2; order[2] = 0; }
        for (int k = 0; k < 4; ++k) { float v = op.clear[order[k]]; v = v < 0 ? 0 : (v > 1 ? 1 : v); texel[k] = (uint8_t)(v * 255.0f + 0.5f); }
    } else {
        bool zero = op.clear[0] == 0 && op.clear[1] == 0 && op.clear[2] == 0 && op.clear[3] == 0;
        if (!zero) { gpu_fail("GPU_OpClearColorF: non-zero clears of format %d are not implemented", (int)t->base.format); return; }
    }
    if (fill_texel_ok(tb)) {
        int rc = pbrk_fill_pattern(p, bytes, texel.data(), (int)tb, st);
        if (rc != PBRK_OK) gpu_fail("clear launch failed (%d)", rc);
    } else {
        std::vector<uint8_t> host(bytes);
        for (size_t o = 0; o < bytes; o += tb) memcpy(host.data() + o, texel.data(), tb);
        HIP_OK(hipMemcpyAsync(p, host.data(), bytes, hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));      // the staging vector dies at scope exit
    }
}

// What an op reads and writes, at whole-texture granularity: the one switch over op kind and kernel that names textures.  A new op
// kind gets one case here; exec_op (what goes stale), graph_replayable (a shade op that would rebuild twins inside a capture) and
// op_access (frames in flight) follow.  Every texture bound in a set counts as read, a bound buffer as memory not followed here.
struct OpEffects {
    TextureImpl* reads[16]; TextureImpl* writes[8]; int n_reads = 0, n_writes = 0;   // writes: a geometry job has five colour targets and its depth
    bool unfollowed = false;                                                  // also touches memory not followed here: buffers, host pointers
    void read(TextureImpl* t) { if (t && n_reads < 16) reads[n_reads++] = t; else if (t) unfollowed = true; }   // more reads than fit: as good as not followed
    void write(TextureImpl* t) { if (t && n_writes < 8) writes[n_writes++] = t; else if (t) gpu_fail("an op writes more than 8 textures"); }
    void bound(const GPU_DescriptorSet* set) { if (set) for (const Slot& sl : set->slots) { if (sl.buf) unfollowed = true; read(sl.tex); } else unfollowed = true; }
};
static OpEffects op_effects(const Op& op) {
    OpEffects e;
    switch (op.kind) {
    case Op_Dispatch:                                                          // stores to one storage image: the sweep's grid, the output of K1 / K3 / K4
        e.bound(op.set);
        if (Slot* out = op.set ? named_slot(op.set, op.cpipe->kernel == Kernel_LightgridSweep ? "IMG0" : "OUTPUT") : nullptr) e.write(out->tex);
        break;
    case Op_Shade: case Op_Raster:
        if (op.kind == Op_Shade) e.bound(op.set); else for (const RasterDraw& d : op.draws) e.bound(d.set);
        e.read(op.blend_tex);                                                  // a folded blit's source (fold_blits)
        if (op.pass) for (const GPU_TextureView& tv : op.pass->targets) e.write((TextureImpl*)tv.texture); else e.unfollowed = true;
        if (op.kind == Op_Raster) e.write(op.tex);                             // the depth target (K14: the light grid)
        if (op.buf) e.unfollowed = true;                                       // SH9 coefficients of a lighting draw; a raster job's vertices
        break;
    case Op_MipGen: e.read(op.tex); e.write(op.tex); break;
    case Op_Blit: e.read(op.tex); e.write(op.tex2); break;                     // folded too: its consumer stores the sum to tex2
    case Op_Clear: case Op_BrdfLutGGX: e.write(op.tex); break;                 // K22 reads its table only: the graph's, written at record time
    case Op_CopyB2T: case Op_IrradianceSH9: case Op_DecodeBC6H: e.write(op.tex); e.unfollowed = true; break;   // from a buffer
    case Op_CopyT2B: case Op_CopyDecodedT2B: case Op_ProjectSH9: case Op_EncodeBC6H: e.read(op.tex); e.unfollowed = true; break;   // into one
    case Op_CopyB2B: e.unfollowed = true; break;
    case Op_CubeToPanorama: case Op_PrefilterGGX: e.read(op.tex); e.write(op.tex2); break;   // their tables belong to the graph and are written at record time only
    }
    return e;
}

static void exec_op(GPU_Graph* g, Op& op, size_t& ev_used) {
    switch (op.kind) {
    case Op_Dispatch:
        if (op.cpipe->kernel == Kernel_LightgridSweep) exec_sweep(g, op, ev_used);
        else if (op.cpipe->kernel == Kernel_BrdfLut) exec_brdf_lut(g, op, ev_used);
        else exec_ibl_filter(g, op, ev_used);                                // K3, K4a, K4b
        break;
    case Op_Shade:
        if (is_bloom_kernel(op.gpipe->kernel)) exec_bloom(g, op, ev_used);
        else if (op.gpipe->kernel == Kernel_TaaResolve) exec_taa(g, op, ev_used);
        else if (op.gpipe->kernel == Kernel_FinalPost) exec_final(g, op, ev_used);
        else exec_shade(g, op, ev_used);                                     // K5, or K16 when the Globals ask for it
        break;
    case Op_Raster: exec_raster(g, op, ev_used); break;
    case Op_MipGen: exec_mipgen(g, op, ev_used); break;
    case Op_Blit: exec_blit(g, op, ev_used); break;
    case Op_Clear: exec_clear(g, op, ev_used); break;
    case Op_CopyB2B: case Op_CopyB2T: case Op_CopyT2B: case Op_CopyDecodedT2B: exec_copy(g, op, ev_used); break;
    case Op_ProjectSH9: case Op_IrradianceSH9: exec_sh9(g, op, ev_used); break;
    case Op_EncodeBC6H: exec_bc6h(g, op, ev_used); break;
    case Op_DecodeBC6H: exec_bc6h_decode(g, op, ev_used); break;
    case Op_CubeToPanorama: exec_panorama(g, op, ev_used); break;
    case Op_PrefilterGGX: exec_prefilter_ggx(g, op, ev_used); break;
    case Op_BrdfLutGGX: exec_brdf_lut_ggx(g, op, ev_used); break;
    }
    const OpEffects e = op_effects(op);                                        // whatever was built from the old bytes is stale now
    for (int i = 0; i < e.n_writes; ++i) texture_written(e.writes[i]);
}

// ---- hipGraph replay of the per-frame chain --------------------------------------------------------------------------
// A frame of the reference records ~25 dependent small launches (light-grid sweep, shade, TAA resolve, 12 bloom passes, tone map:
// render.cpp:1061-1187) into one GPU_Graph and submits it; on a HIP stream each dependent launch costs ~2.7 us of dispatch latency,
// inside an instantiated hipGraph ~2.0 us (tools/ubench_graph.hip).  With replay on, GPU_GraphSubmit captures the op loop of an
// eligible graph into a hipGraph, updates the executable graph kept from the previous submission of the same GPU_Graph in place
// (hipGraphExecUpdate: same topology, new kernel arguments -- the Globals snapshot, the ping-pong targets) or instantiates a new one,
// and launches that.  Eligible = every op is a launch-only op whose lazily built inputs (aprons, cells twins, tables) already
// exist: nothing inside a capture may allocate or synchronise.  Anything else -- the precompute with its side streams, the first
// frame that still builds twins, per-op timing -- takes the plain path.
static bool op_replayable(const Op& op) {
    switch (op.kind) {
    case Op_Dispatch: return op.cpipe->kernel == Kernel_LightgridSweep;
    case Op_MipGen: return true;
    case Op_Blit: return true;
    case Op_CopyB2B: case Op_CopyB2T: case Op_CopyT2B: case Op_CopyDecodedT2B: return false;          // host pointers may be involved: keep them out of captures
    case Op_Raster: return false;                                             // its draw table is uploaded from pinned staging at submit
    case Op_ProjectSH9: case Op_IrradianceSH9: return true;                   // plain launches on device-visible pointers; the scratch exists since recording
    case Op_EncodeBC6H: return true;                                          // one plain launch, texture -> device-visible buffer
    case Op_DecodeBC6H: return true;                                          // the same, buffer -> texture
    case Op_BrdfLutGGX: return true;                                          // one plain launch; its table exists since recording
    case Op_CubeToPanorama: case Op_PrefilterGGX: return false;               // may build the cube's apron (allocation) when they execute
    case Op_Clear: return fill_texel_ok(op.tex->texel_bytes);
    case Op_Shade: {
        if (is_post_kernel(op.gpipe->kernel)) return true;
        ShadeTwin tw[5];
        const int n = shade_twins(op.set, op.gpipe->shade_flags, tw, op.buf != nullptr);
        for (int i = 0; i < n; ++i) if (!shade_twin_ready(tw[i])) return false;
        return named_slot(op.set, "GLOBALS")->buf->pinned_host;
    }
    }
    return false;
}

static bool contains(const std::vector<TextureImpl*>& v, const TextureImpl* t) { for (const TextureImpl* x : v) if (x == t) return true; return false; }
// Graph-level eligibility.  op_replayable() looks at the sampler twins as they are NOW; an earlier op of the same graph that writes
// one of the maps a later shade op samples (exec_op drops the twins of every texture an op writes) would have that shade op rebuild
// its twins -- allocation + synchronisation -- inside the capture.  Such a graph takes the plain path: the textures
// written by the ops seen so far (op_effects) are compared with what each shade op samples.
static bool graph_replayable(GPU_Graph* g) {
    std::vector<TextureImpl*> written;
    for (const Op& op : g->ops) {
        if (!op_replayable(op)) return false;
        if (op.kind == Op_Shade && !is_post_kernel(op.gpipe->kernel)) {
            ShadeTwin tw[5];                                                   // all three maps, whatever the op's flags: a bound map counts even when it is not sampled
            const int n = shade_twins(op.set, GPUX_Shade_IBL, tw);
            for (int i = 0; i < n; ++i) if (contains(written, tw[i].tex)) return false;
        }
        const OpEffects e = op_effects(op);
        written.insert(written.end(), e.writes, e.writes + e.n_writes);
    }
    return true;
}

GPU_API void GPUX_SetGraphReplay(int enable) { G.replay = enable < 0 ? -1 : (enable != 0); }
GPU_API void GPUX_GraphReplayStats(GPU_Graph* g, uint64_t* launches, uint64_t* updates, uint64_t* instantiations) {
    if (!g) return;
    if (launches) *launches = g->replay_launches;
    if (updates) *updates = g->replay_updates;
    if (instantiations) *instantiations = g->replay_instantiations;
}

// The reference's bloom chain copies the TAA result into level 0 of bloom_upscale_rt (a 1:1 GPU_OpBlit, render.cpp:1158-1163) and, five
// passes later, ADDS the last upsample onto that copy (additive blending, render.cpp:1165-1176).  Nothing else reads the copy: the
// upsample can add onto the blit's SOURCE and write the sum to the target, and the copy (33 MB of traffic, one launch per 1080p frame)
// need not exist.  Folded only when the ops between the two provably touch neither subresource: bloom draws with other sources and
// targets; anything else in between keeps the blit.  Same values, same additions: the target's bits do not change.
// A submit-time setting: what its GPUX_Set* call stored in `cached`, else the environment's value or `dflt`, read once on first use
static int env_setting(int& cached, const char* name, int dflt) {
    if (cached < 0) { const char* e = getenv(name); cached = e ? atoi(e) : dflt; }
    return cached;
}
static bool overlap_enabled() { return env_setting(G.overlap, "PBR_GRAPH_OVERLAP", 1) != 0; }
static bool replay_enabled() { return env_setting(G.replay, "PBR_GRAPH_REPLAY", 0) != 0; }

static uint64_t g_folded_blits = 0;
GPU_API uint64_t GPUX_FoldedBlitCount(void) { return g_folded_blits; }
static void fold_blits(GPU_Graph* g) {
    for (Op& op : g->ops) { op.folded = false; op.blend_tex = nullptr; op.skip_level0 = false; }
    if (!env_setting(G.fold, "PBR_GRAPH_FOLD", 1)) return;
    for (size_t i = 0; i < g->ops.size(); ++i) {
        Op& b = g->ops[i];
        // a clear of ALL levels directly followed by a whole-level copy onto level 0 (render.cpp:1156-1163): level 0 -- three quarters of
        // the bytes -- is overwritten before anything can read the zeros
        if (b.kind == Op_Blit && b.size && i > 0 && b.mip2 == 0 && b.tex2->base.layer_count == 1 && b.tex2->base.mip_level_count > 1) {
            Op& c = g->ops[i - 1];
            if (c.kind == Op_Clear && c.tex == b.tex2 && c.mip == GPU_MIP_LEVEL_ALL && b.tex != b.tex2) c.skip_level0 = true;
        }
        if (b.kind != Op_Blit || !b.size || b.layer0 != 0 || b.layer2 != 0 || b.tex->base.layer_count != 1 || b.tex2->base.layer_count != 1 ||
            b.tex->base.format != GPU_Format_RGBA16F || b.tex == b.tex2) continue;
        for (size_t j = i + 1; j < g->ops.size(); ++j) {
            Op& d = g->ops[j];
            if (d.kind != Op_Shade || !is_bloom_kernel(d.gpipe->kernel)) break;
            TextureImpl* target = (TextureImpl*)d.pass->targets[0].texture;
            Slot* in = named_slot(d.set, "TEX0");
            if (!in || !in->tex) break;
            const bool reads_copy = in->tex == b.tex2 && d.mip == b.mip2, writes_src = target == b.tex && d.mip2 == b.mip;
            if (reads_copy || writes_src) break;
            if (target == b.tex2 && d.mip2 == b.mip2) {
                const uint32_t H = mip_dim(target->base.height, d.mip2);
                if (d.gpipe->kernel == Kernel_BloomUp && d.gpipe->blend_additive && d.row0 == 0 && d.row1 == H && !(in->tex == b.tex && d.mip == b.mip)) {
                    b.folded = true; d.blend_tex = b.tex; d.blend_mip = b.mip; ++g_folded_blits;
                }
                break;
            }
        }
    }
}

// op_effects for the frames-in-flight analysis: appends what the op reads and writes; false (ends the walk): not all of it is followed
static bool op_access(const Op& op, std::vector<TextureImpl*>& r, std::vector<TextureImpl*>& w) {
    const OpEffects e = op_effects(op);
    r.insert(r.end(), e.reads, e.reads + e.n_reads);
    w.insert(w.end(), e.writes, e.writes + e.n_writes);
    if (op.kind == Op_Dispatch) w.insert(w.end(), e.reads, e.reads + e.n_reads);   // more cautious than the facts: any texture bound to a dispatch may be a storage image
    return !e.unfollowed;
}
static uint64_t g_overlapped_submits = 0;
GPU_API void GPUX_SetGraphOverlap(int on) { G.overlap = on; }
GPU_API uint64_t GPUX_OverlappedSubmitCount(void) { return g_overlapped_submits; }

// ---- GPU_GraphSubmit, step by step ----
// Submission order is execution order, as on the reference's single queue (vkQueueSubmit, gpu_vulkan.c:2481-2530): a graph
// submitted while another one is still in flight (main.cpp:49-51, 91-99 keeps two) starts after everything enqueued so far on
// the previous graph's stream -- its kernels, lazily built sampler twins, and any exchange the caller appended through
// GPUX_GraphStream.  Side streams fork from g->stream, so they inherit the dependency.
// Frames in flight (main.cpp:49-51, 91-99 keeps two graphs): the tail of a frame's graph -- its bloom chain, a dozen small dependent
// launches that leave most of the chip idle -- touches only the bloom targets, the TAA result it reads and the backbuffer.  The next
// graph's leading ops (light-grid sweep, shade, TAA resolve) touch none of those: they wait for the event in front of the previous
// graph's first bloom draw instead of for its end, and run beside that tail; the first op that shares a texture with the tail (and
// everything behind it) waits for the end as before.  Whole-texture granularity, every texture bound to an op counts; an op this
// analysis does not follow ends the overlap.  PBR_GRAPH_OVERLAP=0: every graph waits for all of its predecessor.
struct OrderPoint {
    GPU_Graph* prev = nullptr;       // set: ops [0, before) wait for prev's mid event only; the wait for its end is still to be enqueued
    size_t before = 0;               // index of the first op that must wait for the previous graph's end
};
static OrderPoint order_after_previous(GPU_Graph* g) {
    OrderPoint o;
    GPU_Graph* prev = G.last_submitted;
    G.last_submitted = g;
    if (!env_setting(G.order, "PBR_GRAPH_ORDER", 1) || !prev || prev == g) return o;
    if (!prev->order_ev) HIP_OK(hipEventCreateWithFlags(&prev->order_ev, hipEventDisableTiming));
    HIP_OK(hipEventRecord(prev->order_ev, prev->stream));
    if (overlap_enabled() && prev->mid_recorded && !replay_enabled()) {
        std::vector<TextureImpl*> r, w;
        for (; o.before < g->ops.size(); ++o.before) {
            r.clear(); w.clear();
            if (!op_access(g->ops[o.before], r, w)) break;
            bool clash = false;
            for (TextureImpl* t : w) clash |= contains(prev->tail_reads, t) || contains(prev->tail_writes, t);
            for (TextureImpl* t : r) clash |= contains(prev->tail_writes, t);
            if (clash) break;
        }
    }
    if (o.before > 0) { HIP_OK(hipStreamWaitEvent(g->stream, prev->mid_ev, 0)); o.prev = prev; ++g_overlapped_submits; }
    else HIP_OK(hipStreamWaitEvent(g->stream, prev->order_ev, 0));
    return o;
}

// This graph's own head / tail split: the tail starts at the first bloom draw.  Returns its index (the op count: no split) and leaves
// what the tail touches in g->tail_reads / g->tail_writes for the next submission's order_after_previous.
static size_t split_head_tail(GPU_Graph* g, bool overlap_on) {
    size_t mid_idx = g->ops.size();
    for (size_t i = 0; i < g->ops.size(); ++i)
        if (g->ops[i].kind == Op_Shade && is_bloom_kernel(g->ops[i].gpipe->kernel)) { mid_idx = i; break; }
    g->mid_recorded = false; g->tail_reads.clear(); g->tail_writes.clear();
    if (!overlap_on || mid_idx == 0) return g->ops.size();
    bool known = true;
    for (size_t i = mid_idx; i < g->ops.size() && known; ++i) known = op_access(g->ops[i], g->tail_reads, g->tail_writes);
    if (!known) { mid_idx = g->ops.size(); g->tail_reads.clear(); g->tail_writes.clear(); }
    return mid_idx;
}

// Precompute dispatches (K3, K4a, K4b) that do not depend on each other run side by side on side streams, fenced by one fork event
// before the first and one join event per stream after the last.  Independent means: outputs disjoint by (texture, mip, faces, rows),
// and no dispatch samples a texture another dispatch of the region writes.  Everything else stays in recording order.
// Two kinds of region:
//   shares -- row-ranged dispatches of less than a whole level (the work units of a partitioned job) are too small to keep 256 CUs x 8
//     waves busy one at a time: consecutive ones go round-robin onto all side streams as they come.  A whole level that follows joins
//     the open region.
//   whole levels -- a job on one GPU is a chain of whole levels (GPUX_OpDispatchRows over every row, or GPU_OpDispatch), none of which
//     reads another, yet in a chain each waits for the last workgroup of the one before: the small levels leave most of the chip idle
//     and every big launch ends in a ragged round.  A run of at least two independent whole levels is taken as one region
//     (level_run): their twins are built ahead of the fork, the dispatches are sorted by cost (samples per texel x texels) and each
//     goes, largest first, onto the least loaded of `n_level` streams: the graph's own and n_level - 1 side streams, so that two
//     streams cost one fork wait and one join: 0.012 ms, measured as the span of a job of two tiny levels with the overlap on
//     against off (profiles/level_streams.md, where the stream count is measured too).
//     GPUX_SetLevelOverlap(0) keeps whole levels in their chain; GPUX_LevelOverlapCount counts the dispatches placed this way.
// Timing: an op's event pair is recorded on the stream it runs on, so inside a region its time is its span BESIDE its neighbours, and
// the sum of the ops exceeds the job: GPUX_GraphSpanMs is the job's figure.  For per-kernel times, profile with the overlap off.
static uint32_t g_level_overlap_count = 0;
struct TileRegion {
    struct Wr { TextureImpl* t; uint32_t mip, f0, f1, r0, r1; };
    GPU_Graph* g;
    int n_side, n_level;
    std::vector<Wr> writes; std::vector<TextureImpl*> reads;       // what the dispatches of the open region write and read
    bool open = false; size_t rr = 0, n_open = 0;                  // n_open: side streams the open region forked

    explicit TileRegion(GPU_Graph* graph) : g(graph) {
        env_setting(G.tile_streams, "PBR_TILE_STREAMS", 4);
        if (G.tile_streams > 16) G.tile_streams = 16;
        n_side = G.tile_streams;
        n_level = !G.level_overlap ? 0 : (G.level_streams < 2 ? kLevelStreams : G.level_streams);
        if (n_level > n_side) n_level = n_side;
    }
    void fork(size_t n) {
        while ((int)g->side.size() > n_side) { (void)hipStreamSynchronize(g->side.back()); (void)hipStreamDestroy(g->side.back()); g->side.pop_back(); }
        while ((int)g->side.size() < n_side) { hipStream_t s; HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); g->side.push_back(s); }
        hipEvent_t e = next_sync_event(g);
        HIP_OK(hipEventRecord(e, g->stream));
        for (size_t s = 0; s < n; ++s) HIP_OK(hipStreamWaitEvent(g->side[s], e, 0));
        open = true; n_open = n;
    }
    // join: the main stream goes on after everything the side streams hold
    void close() {
        if (!open) return;
        for (size_t s = 0; s < n_open; ++s) { hipEvent_t e = next_sync_event(g); HIP_OK(hipEventRecord(e, g->side[s])); HIP_OK(hipStreamWaitEvent(g->stream, e, 0)); }
        writes.clear(); reads.clear(); open = false; g->cur = g->stream;
    }
    // is the op a K3 / K4 dispatch with an output and a source?  `whole`: it covers every face and row of its level
    static bool ibl_dispatch(const Op& op, Slot*& out, Slot*& env, bool& whole) {
        out = env = nullptr; whole = false;
        if (!(op.kind == Op_Dispatch && (op.cpipe->kernel == Kernel_Prefilter || op.cpipe->kernel == Kernel_Irradiance))) return false;
        out = named_slot(op.set, "OUTPUT");
        env = named_slot(op.set, "TEX_ENV_CUBE");
        if (!(out && env && out->tex && env->tex)) return false;
        whole = op.face0 == 0 && op.face1 == out->tex->base.layer_count && op.row0 == 0 && op.row1 == mip_dim(out->tex->base.width, out->mip);
        return true;
    }
    static double evaluations(const Op& op, const Slot* out) {
        return (double)(op.face1 - op.face0) * (op.row1 - op.row0) * mip_dim(out->tex->base.width, out->mip) * dispatch_samples_per_texel(op);
    }
    // does a dispatch that writes `w` and samples `env` depend on, or feed, what the region holds?
    bool clashes(const Wr& w, const TextureImpl* env) const {
        bool clash = w.t == env;
        for (const Wr& o : writes) {
            if (o.t == env) clash = true;
            if (o.t == w.t && o.mip == w.mip && o.f0 < w.f1 && w.f0 < o.f1 && o.r0 < w.r1 && w.r0 < o.r1) clash = true;
        }
        for (TextureImpl* r : reads) if (r == w.t) clash = true;
        return clash;
    }
    // Picks the stream the op launches on (g->cur): a side stream of the shares region (true) -- opening one, or closing it first when
    // the op clashes with what the region holds -- or, behind a closed region, the main stream (false).  The caller sets g->cur back.
    bool place(const Op& op) {
        Slot* out; Slot* env; bool whole;
        // a share of several full-chip rounds (2048 resident workgroups x 256 texels x 8192 samples each) gains nothing from company
        // and keeps its own event timing clean: only smaller ones are overlapped; a whole level does not open a region by itself
        bool tile = n_side >= 2 && ibl_dispatch(op, out, env, whole) && (whole ? open : op.rows_explicit && evaluations(op, out) < 2.0e6 * 8192.0);
        if (!tile) { close(); return false; }
        Wr w = {out->tex, out->mip, op.face0, op.face1, op.row0, op.row1};
        if (clashes(w, env->tex)) close();
        if (w.t == env->tex || (whole && !open)) return false;             // reads what it writes: never overlapped; a whole level opens none
        if (!open) fork((size_t)n_side);
        writes.push_back(w); reads.push_back(env->tex);
        g->cur = g->side[rr++ % g->side.size()];
        return true;
    }
    // With no region open: the end of the run of independent whole levels that starts at op i and stays below `limit`, when it
    // holds at least two (one fork and one join are paid per region, not per dispatch); i otherwise.
    size_t level_run(size_t i, size_t limit) {
        if (open || n_level < 2) return i;
        size_t j = i;
        for (; j < limit; ++j) {
            const Op& op = g->ops[j];
            Slot* out; Slot* env; bool whole;
            if (!ibl_dispatch(op, out, env, whole) || !whole) break;
            Wr w = {out->tex, out->mip, op.face0, op.face1, op.row0, op.row1};
            if (clashes(w, env->tex)) break;
            writes.push_back(w); reads.push_back(env->tex);
        }
        writes.clear(); reads.clear();
        return j - i >= 2 ? j : i;
    }
    // Runs ops [i, j), a run level_run found, as one region.  The twins they sample are built first, in recording order on the main
    // stream: the fork publishes them to every stream, and no stream waits for another inside the region.
    void run_levels(size_t i, size_t j, size_t& ev_used) {
        typedef std::pair<size_t, size_t> Range;                            // timed entries [first, second) of g->timed_names
        const size_t base = g->timed_names.size();
        std::vector<Range> twins(j - i), launch(j - i);
        std::vector<std::pair<double, size_t>> by_cost;
        for (size_t k = i; k < j; ++k) {
            Slot* out; Slot* env; bool whole;
            ibl_dispatch(g->ops[k], out, env, whole);
            twins[k - i].first = g->timed_names.size();
            prepare_ibl_twins(g, g->ops[k], ev_used);
            twins[k - i].second = g->timed_names.size();
            by_cost.push_back({evaluations(g->ops[k], out), k});
        }
        std::stable_sort(by_cost.begin(), by_cost.end(), [](const std::pair<double, size_t>& a, const std::pair<double, size_t>& b) { return a.first > b.first; });
        std::vector<double> load(std::min((size_t)n_level, j - i), 0.0);   // [0]: the graph's own stream, which needs no fork and no join
        fork(load.size() - 1);
        for (const std::pair<double, size_t>& c : by_cost) {
            const size_t s = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());
            load[s] += c.first;
            g->cur = s ? g->side[s - 1] : g->stream;
            launch[c.second - i].first = g->timed_names.size();
            exec_op(g, g->ops[c.second], ev_used);
            launch[c.second - i].second = g->timed_names.size();
        }
        g_level_overlap_count += (uint32_t)(j - i);
        close();
        // The timed ops are reported in recording order, each behind the twins it had built, as in a serial chain: entry e owns the
        // events g->ev[2e] and g->ev[2e + 1] (timed), so names and event pairs are permuted together.
        if (g->timed_names.size() == base) return;
        std::vector<std::string> names; std::vector<hipEvent_t> evs;
        for (size_t k = 0; k < j - i; ++k)
            for (const Range& r : {twins[k], launch[k]})
                for (size_t e = r.first; e < r.second; ++e) { names.push_back(g->timed_names[e]); evs.push_back(g->ev[2 * e]); evs.push_back(g->ev[2 * e + 1]); }
        std::copy(names.begin(), names.end(), g->timed_names.begin() + (ptrdiff_t)base);
        std::copy(evs.begin(), evs.end(), g->ev.begin() + (ptrdiff_t)(2 * base));
    }
};

// hipGraph replay: is this submission captured?  (G.timing and capture exclude each other, so the span events stay outside.)
static bool begin_capture(GPU_Graph* g) {
    if (!replay_enabled() || G.timing || g->replay_broken || g->ops.empty() || !graph_replayable(g)) return false;
    if (hipStreamBeginCapture(g->stream, hipStreamCaptureModeRelaxed) == hipSuccess) return true;
    (void)hipGetLastError(); g->replay_broken = true;
    return false;
}
// Ends the capture; updates the executable graph kept from the previous submission or instantiates a new one, and launches it.
static void finish_capture(GPU_Graph* g, size_t& ev_used) {
    hipGraph_t cg = nullptr;
    bool ok = hipStreamEndCapture(g->stream, &cg) == hipSuccess && cg;
    if (g->exec && g->exec_sig != g->launch_sig) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }   // another kernel behind a node: never "updated"
    if (ok && g->exec) {
        hipGraphNode_t bad = nullptr; hipGraphExecUpdateResult res;
        if (hipGraphExecUpdate(g->exec, cg, &bad, &res) == hipSuccess) ++g->replay_updates;
        else { (void)hipGetLastError(); (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }
    }
    if (ok && !g->exec) {
        if (hipGraphInstantiate(&g->exec, cg, nullptr, nullptr, 0) == hipSuccess) { ++g->replay_instantiations; g->exec_sig = g->launch_sig; }
        else { (void)hipGetLastError(); g->exec = nullptr; ok = false; }
    }
    if (ok && hipGraphLaunch(g->exec, g->stream) == hipSuccess) ++g->replay_launches; else ok = false;
    if (cg) (void)hipGraphDestroy(cg);
    if (ok) return;
    // nothing of the captured work has run: take the plain path for this and every later submission of this graph
    (void)hipGetLastError();
    g->replay_broken = true;
    if (g->exec) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }
    for (Op& op : g->ops) exec_op(g, op, ev_used);
}

GPU_API void GPU_GraphSubmit(GPU_Graph* g) {
    GPU_REQUIRE_V(g && !g->submitted, "GPU_GraphSubmit: graph is NULL or already submitted");
    GPU_REQUIRE_V(g->in_pass == nullptr && g->preparing == nullptr, "GPU_GraphSubmit: render pass still open");
    if (!snapshot_raster_draws(g)) return;
    g->timed_names.clear(); g->timed_ms.clear();
    size_t ev_used = 0;
    g->sync_used = 0;
    g->launch_sig.clear();
    g->cur = g->stream;
    fold_blits(g);
    OrderPoint order = order_after_previous(g);
    const size_t mid_idx = split_head_tail(g, overlap_enabled());
    // the chain property the next submission relies on: this graph's mid event (or, without one, its end) implies the END of the graph
    // before it -- so the wait for that end never comes later than the mid event
    if (order.before > mid_idx) order.before = mid_idx;
    g->span_recorded = false;
    if (G.timing) {
        if (!g->span_a) { HIP_OK(hipEventCreate(&g->span_a)); HIP_OK(hipEventCreate(&g->span_b)); }
        HIP_OK(hipEventRecord(g->span_a, g->stream));
    }
    const bool capture = begin_capture(g);
    TileRegion region(g);
    g_level_overlap_count = 0;
    for (size_t i = 0; i < g->ops.size(); ++i) {
        if (order.prev && i == order.before) {                         // from here on: after everything the previous graph enqueued
            region.close();
            HIP_OK(hipStreamWaitEvent(g->stream, order.prev->order_ev, 0));
            order.prev = nullptr;
        }
        if (i == mid_idx && !capture) {                                // head done: the next graph's independent ops may start
            region.close();
            if (!g->mid_ev) HIP_OK(hipEventCreateWithFlags(&g->mid_ev, hipEventDisableTiming));
            HIP_OK(hipEventRecord(g->mid_ev, g->stream));
            g->mid_recorded = true;
        }
        // a run of whole levels stays on one side of the previous graph's end (it has none of this graph's bloom draws in it)
        const size_t run_end = region.level_run(i, order.prev && i < order.before ? order.before : g->ops.size());
        if (run_end > i) { region.run_levels(i, run_end, ev_used); i = run_end - 1; continue; }
        region.place(g->ops[i]);
        exec_op(g, g->ops[i], ev_used);
        g->cur = g->stream;
    }
    region.close();
    if (order.prev) HIP_OK(hipStreamWaitEvent(g->stream, order.prev->order_ev, 0));   // every op was independent: still end after it
    if (G.timing) { HIP_OK(hipEventRecord(g->span_b, g->stream)); g->span_recorded = true; }
    if (capture) finish_capture(g, ev_used);
    g->submitted = true;
}

GPU_API void GPU_GraphWait(GPU_Graph* g) {
    GPU_REQUIRE_V(g, "GPU_GraphWait: NULL graph");
    HIP_OK(hipStreamSynchronize(g->stream));
    g->timed_ms.clear();
    for (size_t i = 0; i < g->timed_names.size(); ++i) {
        float ms = 0.0f;
        HIP_OK(hipEventElapsedTime(&ms, g->ev[2 * i], g->ev[2 * i + 1]));
        g->timed_ms.push_back(ms);
    }
    g->span_ms = 0.0f;
    if (g->span_recorded) { HIP_OK(hipEventElapsedTime(&g->span_ms, g->span_a, g->span_b)); g->span_recorded = false; }
    reset_graph(g);                      // Wait also resets the graph [gpu.h:452]
}

GPU_API void GPUX_EnableOpTiming(int enable) { G.timing = enable != 0; }
GPU_API void GPUX_SetTileStreams(int count) { G.tile_streams = count < 0 ? -1 : count; }
GPU_API void GPUX_SetLevelOverlap(int on) { G.level_overlap = on != 0; }
GPU_API void GPUX_SetLevelStreams(int count) { G.level_streams = count < 2 ? -1 : count; }
GPU_API uint32_t GPUX_LevelOverlapCount(void) { return g_level_overlap_count; }
GPU_API uint32_t GPUX_GraphTimedOpCount(GPU_Graph* g) { return g ? (uint32_t)g->timed_ms.size() : 0; }
GPU_API const char* GPUX_GraphTimedOpName(GPU_Graph* g, uint32_t i) { return (g && i < g->timed_names.size()) ? g->timed_names[i].c_str() : ""; }
GPU_API float GPUX_GraphTimedOpMs(GPU_Graph* g, uint32_t i) { return (g && i < g->timed_ms.size()) ? g->timed_ms[i] : 0.0f; }
GPU_API float GPUX_GraphSpanMs(GPU_Graph* g) { return g ? g->span_ms : 0.0f; }
GPU_API void GPUX_SetPrefilterTolerance(float rel) { G.prefilter_tol = rel > 0.0f ? rel : 0.0f; }
GPU_API int GPUX_PrefilterKeptSamples(uint32_t mip) { return mip < 32 ? G.kept_samples[mip] : 0; }
