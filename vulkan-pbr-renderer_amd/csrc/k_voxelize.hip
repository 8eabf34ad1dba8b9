// k_voxelize.hip -- K14: the voxelise pass, shaders/lightgrid_voxelize.glsl (render.cpp:1039-1056), as a compute rasteriser.
//
// The pass draws every triangle along its dominant axis into an N x N target with conservative rasterisation and stores one lit
// colour per fragment into the N^3 light grid.  Which of several stores to one voxel wins is fixed by the contract:
// the largest (triangle number, pixel row, pixel column).  A maximum does not depend on execution order, so the pass is
//   * cover   (one lane per triangle): vertex stage and snap (vox_setup), then the lane walks its own conservative pixel box and, for
//             every fragment whose voxel lies in the grid, issues a 64-bit atomicMax of ((triangle + 1) << 16 | row << 8 | column)
//             into an N^3 owner grid in scratch.  Voxelised triangles are a few voxels across; one with a box of more than kSmallBox
//             pixels is appended to a list instead;
//   * large   (one workgroup per listed triangle, the lanes stride over its box);
//   * resolve (one lane per voxel): a voxel with an owner redoes the vertex stage of that triangle, shades that one fragment
//             (vox_shade) and stores 8 bytes.  A voxel nobody addressed keeps its contents.
// No atomics touch the image, kernel boundaries order the phases, and no per-triangle record is kept: the rules live once in
// voxelize_core.h and a triangle is cheaper to set up again than to store and fetch.  Scratch (owner grid, list, its counter) follows
// from the triangle count and N alone.  find_draw and the launch shape come from raster_bins.h.
#include "voxelize_core.h"
#include "raster_bins.h"

#include <hip/hip_fp16.h>

namespace {
constexpr int kSmallBox = 64;             // a lane walks a box of at most this many pixels itself

struct VoxLayout { size_t owner, count, large, total; };

VoxLayout vox_layout(uint32_t n_tri, int N) {
    VoxLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    L.owner = take((size_t)N * N * N * 8);
    L.count = take(4);
    L.large = take((size_t)n_tri * 4);
    L.total = o;
    return L;
}

// the fragment of pixel (i, j) of job triangle t, if there is one and its voxel lies in the grid
__device__ inline unsigned cover_pixel(unsigned long long* owner, const VoxTri& T, uint32_t t, int i, int j, int N) {
    int c[3];
    if (!vox_covers(T, i, j) || !vox_coord(T, i, j, N, c)) return 0u;
    const unsigned long long key = ((unsigned long long)(t + 1) << 16) | ((unsigned long long)j << 8) | (unsigned long long)i;
    atomicMax(&owner[((size_t)c[2] * N + c[1]) * N + c[0]], key);             // in range: 0 <= c < N, checked by vox_coord
    return 1u;
}

// the kept fragments of a wave, one atomic per wave; every lane of the wave calls it
__device__ inline void count_fragments(unsigned long long* counter, unsigned n) {
    if (!counter) return;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(counter, (unsigned long long)n);
}

__global__ __launch_bounds__(kThreads) void k_vox_cover(PbrkVoxelizeArgs a, VoxLayout L) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    char* scratch = (char*)a.scratch;
    bool rejected = false;
    unsigned kept = 0;
    if (t < a.tri_count) {
        const PbrkVoxDraw& d = a.draws[find_draw(a.draws, a.draw_count, t)];
        VoxTri T;
        const int st = vox_setup(d, t - d.first_tri, a.n, T);
        rejected = st < 0;
        if (st > 0) {
            const int w = T.box[2] - T.box[0] + 1, h = T.box[3] - T.box[1] + 1;
            if (w * h <= kSmallBox) {
                unsigned long long* owner = (unsigned long long*)(scratch + L.owner);
                for (int j = T.box[1]; j <= T.box[3]; ++j)
                    for (int i = T.box[0]; i <= T.box[2]; ++i) kept += cover_pixel(owner, T, t, i, j, a.n);
            } else {
                const unsigned slot = atomicAdd((unsigned*)(scratch + L.count), 1u);   // < tri_count
                ((unsigned*)(scratch + L.large))[slot] = t;
            }
        }
    }
    const unsigned long long m = __ballot(rejected);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.rejected, (unsigned long long)__popcll(m));
    count_fragments(a.fragments, kept);
}

__global__ __launch_bounds__(kThreads) void k_vox_large(PbrkVoxelizeArgs a, VoxLayout L) {
    char* scratch = (char*)a.scratch;
    const unsigned n = *(const unsigned*)(scratch + L.count);
    unsigned long long* owner = (unsigned long long*)(scratch + L.owner);
    unsigned kept = 0;
    for (unsigned e = blockIdx.x; e < n; e += gridDim.x) {
        const uint32_t t = ((const unsigned*)(scratch + L.large))[e];
        const PbrkVoxDraw& d = a.draws[find_draw(a.draws, a.draw_count, t)];
        VoxTri T;
        if (vox_setup(d, t - d.first_tri, a.n, T) <= 0) continue;            // the same for every lane of the workgroup
        const int w = T.box[2] - T.box[0] + 1, h = T.box[3] - T.box[1] + 1;
        for (int p = threadIdx.x; p < w * h; p += kThreads) kept += cover_pixel(owner, T, t, T.box[0] + p % w, T.box[1] + p / w, a.n);
    }
    count_fragments(a.fragments, kept);
}

__global__ __launch_bounds__(kThreads) void k_vox_resolve(PbrkVoxelizeArgs a, VoxLayout L) {
    const size_t v = (size_t)blockIdx.x * kThreads + threadIdx.x, nv = (size_t)a.n * a.n * a.n;
    if (v >= nv) return;
    const unsigned long long key = ((const unsigned long long*)((const char*)a.scratch + L.owner))[v];
    if (!key) return;
    const uint32_t t = (uint32_t)(key >> 16) - 1;
    const int j = (int)((key >> 8) & 255u), i = (int)(key & 255u);
    const PbrkVoxDraw& d = a.draws[find_draw(a.draws, a.draw_count, t)];
    VoxTri T;
    if (vox_setup(d, t - d.first_tri, a.n, T) <= 0) return;                   // cannot happen: the key came from this triangle
    float c[3];
    vox_shade(d, T, i, j, c);
    uint2 o;                                                                  // K7's store: RGBA16F, round to nearest even
    o.x = (unsigned)__half_as_ushort(__float2half_rn(c[0])) | ((unsigned)__half_as_ushort(__float2half_rn(c[1])) << 16);
    o.y = (unsigned)__half_as_ushort(__float2half_rn(c[2])) | (0x3c00u << 16);
    ((uint2*)a.grid)[v] = o;
}

bool args_ok(const PbrkVoxelizeArgs* a) {
    return a && a->draws && a->grid && a->scratch && a->rejected && a->draw_count > 0 && a->n >= 8 && a->n <= 256 && (a->n & 7) == 0 &&
           a->tri_count <= (1u << 26);
}
}  // namespace

extern "C" size_t pbrk_voxelize_scratch_bytes(uint32_t tri_count, int n, int n_again) {
    (void)n_again;
    if (n < 8 || n > 256 || (n & 7) || tri_count > (1u << 26)) return 0;
    return vox_layout(tri_count, n).total;
}

extern "C" int pbrk_voxelize_cover(const PbrkVoxelizeArgs* a, void* stream) {
    if (!args_ok(a)) return PBRK_E_ARG;
    if (a->tri_count == 0) return PBRK_OK;
    const VoxLayout L = vox_layout(a->tri_count, a->n);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync((char*)a->scratch, 0, L.large, st) != hipSuccess) return PBRK_E_LAUNCH;      // owner grid and list counter
    hipLaunchKernelGGL(k_vox_cover, dim3((a->tri_count + kThreads - 1) / kThreads), dim3(kThreads), 0, st, *a, L);
    const uint32_t blocks = a->tri_count < 4096u ? a->tri_count : 4096u;     // the list's length stays on the device: a strided loop
    hipLaunchKernelGGL(k_vox_large, dim3(blocks), dim3(kThreads), 0, st, *a, L);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}

extern "C" int pbrk_voxelize_resolve(const PbrkVoxelizeArgs* a, void* stream) {
    if (!args_ok(a)) return PBRK_E_ARG;
    if (a->tri_count == 0) return PBRK_OK;
    const VoxLayout L = vox_layout(a->tri_count, a->n);
    const size_t nv = (size_t)a->n * a->n * a->n;
    hipLaunchKernelGGL(k_vox_resolve, dim3((unsigned)((nv + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, *a, L);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}
