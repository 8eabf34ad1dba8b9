// k_gridview.hip -- K16: the light-grid visualiser of the lighting pass (gfx950).
//
// Replaces the "VOXEL DEBUG RAY TRACER" block of shaders/lighting_pass.glsl (:463-491), which the reference turns on with
// render_params.visualize_lightgrid (main.cpp:79, render.cpp:990) and which then replaces the shading of every pixel, sky included.
// The arithmetic is csrc/gridview_core.h (also compiled for the host by tests/gridview_core_host.cpp); this file adds what makes it
// a kernel:
//   - one pixel per lane in 8 x 8-pixel waves (a 32 x 8 block), as K5's GI instantiation: neighbouring rays stay in neighbouring
//     voxels, and fewer waves straddle a silhouette than with 64 x 1 strips;
//   - the march positions do not depend on what is read (only the exit does), so the taps of GV_AHEAD steps are fetched together and
//     consumed in order: the same values in the same order, GV_AHEAD times fewer dependent round trips;
//   - the march reads the alpha channel alone (2 of a texel's 8 bytes); the three colour channels are fetched once, for the sample
//     that hit.  The channels are filtered independently of each other, so both are the bits of the full sample (grid_sample of
//     k_shade.hip; pbrk_debug_sample which = 3 against which = 0 and the oracle).
// No early termination: a ray that has left the cube keeps sampling clamped edge voxels and can still hit, as in the reference.  The
// loop is bounded by GV_MAX_STEPS, so every wave ends.
#include "k_shade_internal.h"
#include "gridview_core.h"
#include <string.h>

#ifndef GV_AHEAD
#define GV_AHEAD 8
#endif
static_assert(GV_MAX_STEPS % GV_AHEAD == 0, "the march is consumed in whole groups");

struct GridViewParams {
    int width, height, x0, y0, w, h;
    const __half* grid; int n;              // half4 [n][n][n]
    void* out; int out_fmt;
    float wfc[16], cam[3], lightgrid_scale, frame_idx_mod_59;
};

struct GridTaps { unsigned t[8]; float a, b, c; };    // texel indices in z, y, x order (t000, t001, ..), weights along x, y, z
__device__ __forceinline__ GridTaps grid_taps(int n, const float* p) {
    int i0, i1, j0, j1, k0, k1;
    GridTaps g;
    snap_split(p[0], n, i0, i1, g.a); snap_split(p[1], n, j0, j1, g.b); snap_split(p[2], n, k0, k1, g.c);
    g.t[0] = (unsigned)((k0 * n + j0) * n + i0); g.t[1] = (unsigned)((k0 * n + j0) * n + i1);
    g.t[2] = (unsigned)((k0 * n + j1) * n + i0); g.t[3] = (unsigned)((k0 * n + j1) * n + i1);
    g.t[4] = (unsigned)((k1 * n + j0) * n + i0); g.t[5] = (unsigned)((k1 * n + j0) * n + i1);
    g.t[6] = (unsigned)((k1 * n + j1) * n + i0); g.t[7] = (unsigned)((k1 * n + j1) * n + i1);
    return g;
}
// one channel of texture(sampler3D(LIGHTGRID, SAMPLER_LINEAR_CLAMP), p): the lerp tree of grid_sample
__device__ __forceinline__ float grid_channel(const __half* __restrict__ grid, const GridTaps& g, int ch) {
    float t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = __half2float(grid[(size_t)g.t[k] * 4 + ch]);
    return lerp_x(lerp_x(lerp_x(t[0], t[1], g.a), lerp_x(t[2], t[3], g.a), g.b), lerp_x(lerp_x(t[4], t[5], g.a), lerp_x(t[6], t[7], g.a), g.b), g.c);
}
__device__ __forceinline__ float grid_alpha(const __half* __restrict__ grid, int n, const float* p) { return grid_channel(grid, grid_taps(n, p), 3); }
__device__ __forceinline__ void grid_rgb(const __half* __restrict__ grid, int n, const float* p, float* rgb) {
    const GridTaps g = grid_taps(n, p);
    const uint2* __restrict__ tex = (const uint2*)grid;
    float4 t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = unpack_h4(tex[g.t[k]]);
    rgb[0] = lerp_x(lerp_x(lerp_x(t[0].x, t[1].x, g.a), lerp_x(t[2].x, t[3].x, g.a), g.b), lerp_x(lerp_x(t[4].x, t[5].x, g.a), lerp_x(t[6].x, t[7].x, g.a), g.b), g.c);
    rgb[1] = lerp_x(lerp_x(lerp_x(t[0].y, t[1].y, g.a), lerp_x(t[2].y, t[3].y, g.a), g.b), lerp_x(lerp_x(t[4].y, t[5].y, g.a), lerp_x(t[6].y, t[7].y, g.a), g.b), g.c);
    rgb[2] = lerp_x(lerp_x(lerp_x(t[0].z, t[1].z, g.a), lerp_x(t[2].z, t[3].z, g.a), g.b), lerp_x(lerp_x(t[4].z, t[5].z, g.a), lerp_x(t[6].z, t[7].z, g.a), g.b), g.c);
}

__global__ __launch_bounds__(256) void k_gridview(const GridViewParams p) {
    const int lx = blockIdx.x * 32 + (threadIdx.x >> 6) * 8 + (threadIdx.x & 7), ly = blockIdx.y * 8 + ((threadIdx.x >> 3) & 7);
    if (lx >= p.w || ly >= p.h) return;
    const int px = p.x0 + lx, py = p.y0 + ly;
    const float frag_x = (float)px + 0.5f, frag_y = (float)py + 0.5f;          // gl_FragCoord.xy
    const float u = frag_x / (float)p.width, v = frag_y / (float)p.height;     // fs_uv: true divisions
    GvRay r;
    gv_ray(p.wfc, p.cam, p.lightgrid_scale, p.frame_idx_mod_59, u, v, frag_x, frag_y, r);
    bool hit = false;
    float hp[3] = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < GV_MAX_STEPS && !hit; i += GV_AHEAD) {
        float pk[GV_AHEAD][3], ak[GV_AHEAD];
#pragma unroll
        for (int k = 0; k < GV_AHEAD; ++k) {
            gv_step(r, pk[k]);
            ak[k] = grid_alpha(p.grid, p.n, pk[k]);
        }
#pragma unroll
        for (int k = 0; k < GV_AHEAD; ++k)
            if (!hit && gv_hits(ak[k])) { hit = true; hp[0] = pk[k][0]; hp[1] = pk[k][1]; hp[2] = pk[k][2]; }
    }
    float rgb[3] = {0.0f, 0.0f, 0.0f}, o[4];
    if (hit) grid_rgb(p.grid, p.n, hp, rgb);
    gv_resolve(hit, rgb, o);
    const size_t pi = (size_t)py * p.width + px;
    if (p.out_fmt == PBRK_FMT_RGBA16F) {
        __half2 lo = __halves2half2(__float2half_rn(o[0]), __float2half_rn(o[1]));
        __half2 hi = __halves2half2(__float2half_rn(o[2]), __float2half_rn(o[3]));
        uint2 packed;
        packed.x = *reinterpret_cast<unsigned*>(&lo);
        packed.y = *reinterpret_cast<unsigned*>(&hi);
        ((uint2*)p.out)[pi] = packed;
    } else {
        ((float4*)p.out)[pi] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

extern "C" int pbrk_lightgrid_view(const PbrkGridViewArgs* a, void* stream) {
    if (!a || a->width < 1 || a->height < 1) return PBRK_E_ARG;
    if (a->x0 < 0 || a->y0 < 0 || a->x1 > a->width || a->y1 > a->height || a->x0 >= a->x1 || a->y0 >= a->y1) return PBRK_E_ARG;
    if (!a->lightgrid || a->lightgrid_size < 1 || a->lightgrid_size > 1024 || !a->out) return PBRK_E_ARG;
    if (a->out_format != PBRK_FMT_RGBA16F && a->out_format != PBRK_FMT_RGBA32F) return PBRK_E_FORMAT;
    GridViewParams p;
    p.width = a->width; p.height = a->height; p.x0 = a->x0; p.y0 = a->y0; p.w = a->x1 - a->x0; p.h = a->y1 - a->y0;
    p.grid = (const __half*)a->lightgrid; p.n = a->lightgrid_size;
    p.out = a->out; p.out_fmt = a->out_format;
    for (int i = 0; i < 16; ++i) p.wfc[i] = a->globals[32 + i];
    for (int i = 0; i < 3; ++i) p.cam[i] = a->globals[132 + i];
    p.frame_idx_mod_59 = a->globals[135];
    p.lightgrid_scale = a->globals[136];
    hipLaunchKernelGGL(k_gridview, dim3((p.w + 31) / 32, (p.h + 7) / 8), dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}

// diagnostics (pbrk_debug_sample which = 3): K16's channel-split sampler at arbitrary coordinates, (rgb, alpha) put together again
__global__ void k_debug_sample_gridview(const __half* __restrict__ grid, int n, const float* __restrict__ coords, int count, float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float c[3] = {coords[i * 3], coords[i * 3 + 1], coords[i * 3 + 2]};
    float rgb[3];
    grid_rgb(grid, n, c, rgb);
    out[i] = make_float4(rgb[0], rgb[1], rgb[2], grid_alpha(grid, n, c));
}
extern "C" __attribute__((visibility("hidden"))) int pbrk_debug_sample_gridview(const void* texture, int n, const void* coords, int count, void* out, void* stream) {
    hipLaunchKernelGGL(k_debug_sample_gridview, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const __half*)texture, n, (const float*)coords, count, (float4*)out);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}
