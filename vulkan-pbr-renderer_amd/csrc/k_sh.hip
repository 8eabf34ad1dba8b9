// k_sh.hip -- K17: SH9 projection of one cube level and the irradiance cube of nine coefficients, by the contract of
// sh_core.h.  The reference has no counterpart: its only diffuse output is the cube of gen_irradiance_map.glsl (K3).
//
// Projection = a reduction over a whole level, 16 B read per texel, fp64 sums, no floating-point atomics:
//   stage one   a wave owns a tile of 64 columns x R rows and walks it row by row; lane = column, and in every row a lane handles the
//               texel (ix, iy) of ALL requested faces: the six loads of a row (6 x 1 KiB per wave, each one contiguous) are issued
//               before the first is used, and everything that depends on (ix, iy) alone -- domega and 1 / |(1, sc, tc)| -- is computed
//               once for up to six texels.  domega needs A() at the texel's four corners; the walk keeps the two of the row above,
//               computes ONE new corner per lane and row (its lower left) and takes the lower right from the lane to its right; lane 63
//               takes it from a per-tile column of R + 1 edge corners that the lanes computed side by side before the walk.  So a
//               tile costs R + 2 atan2 per lane for up to 6 R texels (0.17 .. 0.21 per texel) instead of 4 per texel, with the
//               bits sh_solid_angle() gives.  Opposite faces share one basis evaluation (sh_pair_texels).  The loads of row iy + 1
//               are issued before row iy is summed: a row is ~350 fp64 instructions per wave, and with three waves per SIMD
//               (launch bound) a load has several microseconds to land.  The 27 sums of a workgroup's 256 lanes are folded by a fixed butterfly within each
//               wave and then wave 0 .. 3 in order: one 27-double partial per workgroup.
//   stage two   one workgroup, thread k adds partial 0, 1, 2, ... of coefficient k: index order, so equal arguments give equal bytes;
//               the loads go 32 at a time (one load and one wait per partial cost 0.3 us each: 0.6 ms of tail behind a 4096^2 level).
// Irradiance: one lane per texel, 27 uniform doubles in, one 16-byte store out.
#include "sh_core.h"
#include "pbr_kernels.h"

#define SH_MAX_N 16384
#ifndef SH_AHEAD
#define SH_AHEAD 2                                                             // rows of loads in flight ahead of the sums
#endif
#ifndef SH_WAVES
#define SH_WAVES 2
#endif

// rows per tile: 32 on big levels (fewest atan2 per texel), fewer on small ones so that the level still spreads over the chip
static int sh_tile_rows(int n) { return n >= 2048 ? 32 : n >= 512 ? 16 : 8; }
static size_t sh_workgroups(int n, int rows) {
    const size_t tiles = (size_t)((n + 63) / 64) * (size_t)((rows + sh_tile_rows(n) - 1) / sh_tile_rows(n));
    return (tiles + 3) / 4;
}

// Faces 2 p and 2 p + 1 at one (sc, tc) are mirror images: (x, y, z) of the second is the first's with two signs flipped (p = 0, 2:
// x and z; p = 1: y and z), so Y_k of the second is +-Y_k of the first, exactly.  One basis evaluation and 27 FMAs then serve two
// texels: coefficient k takes L_first + L_second or L_first - L_second (double; a face outside the requested range enters as 0).
template <int P>
__device__ __forceinline__ void sh_pair_texels(double acc[27], const float3& a, const float3& b, double sc, double tc, double inv, double dw) {
    double d[3], Y[9];
    sh_face_dir(2 * P, sc, tc, inv, d);
    sh_basis(d, Y);
    const double la[3] = {(double)a.x, (double)a.y, (double)a.z}, lb[3] = {(double)b.x, (double)b.y, (double)b.z};
    double sum[3], dif[3];
    for (int c = 0; c < 3; ++c) { sum[c] = la[c] + lb[c]; dif[c] = la[c] - lb[c]; }
    // sign of Y_k under the pair's flip, k = 1, y, z, x, xy, yz, 3zz-1, xz, xx-yy
    constexpr bool even_xz[9] = {true, true, false, false, false, false, true, true, true};
    constexpr bool even_yz[9] = {true, false, false, true, false, true, true, false, true};
    for (int k = 0; k < 9; ++k) {
        const double w = Y[k] * dw;
        const bool even = P == 1 ? even_yz[k] : even_xz[k];
        for (int c = 0; c < 3; ++c) acc[3 * k + c] = fma(even ? sum[c] : dif[c], w, acc[3 * k + c]);
    }
}

__device__ __forceinline__ void sh_load_row(float3 v[6], const float4* __restrict__ level, int n, int face0, int face1, int iy, int ix, bool live) {
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        v[f] = make_float3(0.0f, 0.0f, 0.0f);
        if (live && f >= face0 && f < face1) {
            const float* p = (const float*)(level + ((size_t)f * n + iy) * n);    // wave-uniform row base + a 32-bit lane offset
            const unsigned o = 4u * (unsigned)ix;
            v[f] = make_float3(p[o], p[o + 1], p[o + 2]);
        }
    }
}

__global__ __launch_bounds__(256, SH_WAVES) void k_sh9_partial(const float4* __restrict__ level, int n, int face0, int face1, int y0, int y1,
                                                        int tile_rows, int col_tiles, int tiles, double* __restrict__ partials) {
    __shared__ double wave_sum[4][27];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x * 4 + wave;                                    // wave-uniform
    double acc[27];
    for (int i = 0; i < 27; ++i) acc[i] = 0.0;
    if (tile < tiles) {
        const int tx = tile % col_tiles, ty = tile / col_tiles;
        const int ix = tx * 64 + lane;
        const bool live = ix < n;
        const int r0 = y0 + ty * tile_rows, r1 = min(r0 + tile_rows, y1);      // r0 < r1 <= n
        float3 row[SH_AHEAD + 1][6];                                           // row[0]: the row being summed; row[d]: d rows ahead
#pragma unroll
        for (int d = 0; d < SH_AHEAD; ++d) if (r0 + d < r1) sh_load_row(row[d], level, n, face0, face1, r0 + d, ix, live);
        const double ex = sh_corner(min(ix, n), n);                            // this lane's corner column; lane + 1 holds the next one
        // the corner column right of lane 63, rows r0 .. r0 + tile_rows (<= 33 values): lane l holds row r0 + l
        const double edge = sh_area(sh_corner(min(tx * 64 + 64, n), n), sh_corner(min(r0 + lane, n), n));
        const double sc = sh_centre(min(ix, n - 1), n);
        double a0 = sh_area(ex, sh_corner(r0, n));
        double a0r = __shfl_down(a0, 1);
        { const double e = __shfl(edge, 0); if (lane == 63) a0r = e; }
        for (int iy = r0; iy < r1; ++iy) {                                     // wave-uniform bounds: every lane takes part in the shuffles
            // the loads of row iy + SH_AHEAD (< r1 <= n) are issued before row iy is summed
            if (iy + SH_AHEAD < r1) sh_load_row(row[SH_AHEAD], level, n, face0, face1, iy + SH_AHEAD, ix, live);
            const double a1 = sh_area(ex, sh_corner(iy + 1, n));
            double a1r = __shfl_down(a1, 1);
            { const double e = __shfl(edge, iy + 1 - r0); if (lane == 63) a1r = e; }
            const double dw = sh_solid_angle_of(a0, a1, a0r, a1r);
            const double tc = sh_centre(iy, n), inv = sh_inv_len(sc, tc);
            if (live) {
                if (face0 < 2) sh_pair_texels<0>(acc, row[0][0], row[0][1], sc, tc, inv, dw);
                if (face0 < 4 && face1 > 2) sh_pair_texels<1>(acc, row[0][2], row[0][3], sc, tc, inv, dw);
                if (face1 > 4) sh_pair_texels<2>(acc, row[0][4], row[0][5], sc, tc, inv, dw);
            }
            a0 = a1; a0r = a1r;
#pragma unroll
            for (int d = 0; d < SH_AHEAD; ++d)
#pragma unroll
                for (int f = 0; f < 6; ++f) row[d][f] = row[d + 1][f];
        }
    }
    for (int i = 0; i < 27; ++i) {
        double s = acc[i];
        for (int m = 32; m >= 1; m >>= 1) s = s + __shfl_xor(s, m);
        if (lane == 0) wave_sum[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < 27) {
        const int i = threadIdx.x;
        partials[(size_t)blockIdx.x * 27 + i] = ((wave_sum[0][i] + wave_sum[1][i]) + wave_sum[2][i]) + wave_sum[3][i];
    }
}

// Index order, but not one memory round trip per partial: 32 loads are in flight before the first of them is added.  A slot past the
// end adds +0.0, which changes no sum.
__global__ __launch_bounds__(64) void k_sh9_final(const double* __restrict__ partials, int count, double* __restrict__ out27) {
    const int i = threadIdx.x;
    if (i >= 27) return;
    constexpr int BATCH = 32;
    double s = 0.0;
    for (int p = 0; p < count; p += BATCH) {
        double v[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) v[j] = p + j < count ? partials[(size_t)(p + j) * 27 + i] : 0.0;
#pragma unroll
        for (int j = 0; j < BATCH; ++j) s = s + v[j];
    }
    out27[i] = s;
}

__global__ __launch_bounds__(256) void k_sh9_irradiance(const double* __restrict__ coef27, float4* __restrict__ out, int size,
                                                        int face0, int y0, int y1) {
    const int face = face0 + (int)blockIdx.y;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, count = (size_t)(y1 - y0) * size;
    if (t >= count) return;
    const int iy = y0 + (int)(t / size), ix = (int)(t % size);
    double coef[27];
    for (int i = 0; i < 27; ++i) coef[i] = coef27[i];
    float rgba[4];
    sh_irradiance_texel(coef, size, face, ix, iy, rgba);
    out[((size_t)face * size + iy) * size + ix] = make_float4(rgba[0], rgba[1], rgba[2], rgba[3]);
}

static bool sh_range_ok(int n, int face0, int face1, int y0, int y1) {
    return n >= 1 && n <= SH_MAX_N && face0 >= 0 && face0 < face1 && face1 <= 6 && y0 >= 0 && y0 < y1 && y1 <= n;
}

extern "C" size_t pbrk_sh9_scratch_bytes(int n) {
    if (n < 1 || n > SH_MAX_N) return 0;
    return sh_workgroups(n, n) * 27 * sizeof(double);
}

extern "C" int pbrk_sh9_project(const void* level, int n, int face0, int face1, int y0, int y1, void* scratch, double* out27, void* stream) {
    if (!level || !scratch || !out27 || !sh_range_ok(n, face0, face1, y0, y1)) return PBRK_E_ARG;
    if (((uintptr_t)level % 16) != 0 || ((uintptr_t)scratch % 8) != 0 || ((uintptr_t)out27 % 8) != 0) return PBRK_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int tile_rows = sh_tile_rows(n), col_tiles = (n + 63) / 64;
    const int tiles = col_tiles * ((y1 - y0 + tile_rows - 1) / tile_rows);     // <= 256 x 512
    const int groups = (int)sh_workgroups(n, y1 - y0);                         // <= sh_workgroups(n, n): what the scratch holds
    hipLaunchKernelGGL(k_sh9_partial, dim3((unsigned)groups), dim3(256), 0, st, (const float4*)level, n, face0, face1, y0, y1, tile_rows,
                       col_tiles, tiles, (double*)scratch);
    hipLaunchKernelGGL(k_sh9_final, dim3(1), dim3(64), 0, st, (const double*)scratch, groups, out27);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}

extern "C" int pbrk_sh9_irradiance(const double* coef27, void* out_level, int size, int face0, int face1, int y0, int y1, void* stream) {
    if (!coef27 || !out_level || !sh_range_ok(size, face0, face1, y0, y1)) return PBRK_E_ARG;
    if (((uintptr_t)coef27 % 8) != 0 || ((uintptr_t)out_level % 16) != 0) return PBRK_E_ARG;
    const size_t count = (size_t)(y1 - y0) * size;
    const dim3 grid((unsigned)((count + 255) / 256), (unsigned)(face1 - face0));
    hipLaunchKernelGGL(k_sh9_irradiance, grid, dim3(256), 0, (hipStream_t)stream, coef27, (float4*)out_level, size, face0, y0, y1);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}
