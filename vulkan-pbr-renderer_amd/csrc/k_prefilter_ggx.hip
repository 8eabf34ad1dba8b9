// k_prefilter_ggx.hip -- K21 (an extension: the reference's prefilter is K4b's Beckmann Monte Carlo): one level of the
// specular cube by GGX importance sampling with filtered lookups.  The contract is in prefilter_ggx_core.h.
//
// One texel per lane, 64 texels per wave.  Everything about a sample but the texel's frame is texel-independent, the source levels
// and the blend between them included, so the host hands each kept sample over as two 16-byte entries -- {l.x, l.y, l.z, f} and
// {offset and size of level l0, offset and size of level l1} -- and the loop index is wave-uniform: the entries arrive through the
// scalar cache, and the level bases and sizes live in SGPRs.  Per sample a lane forms d (6 VALU), selects the face and projects
// ONCE (s, t do not depend on the level: two IEEE divisions), takes the four taps of each of the two levels (8 loads of 16 bytes,
// 4 where l1 == l0, a wave-uniform branch) and accumulates RGB.
//
// Levels with too few texels to fill 256 CUs split the samples over S waves of the workgroup (pggx_slices: a function of the
// level's size alone); wave k takes a contiguous run of the table, the partial sums go through LDS and wave 0 adds them in the order
// of k: no atomics, the same bytes every time, whatever face / row range the texel was dispatched in.
#include "pbr_device.h"
#include "pbr_kernels.h"
#include "prefilter_ggx_core.h"

struct GgxParams {
    const float4* src;          // bordered twin of the source, level 0 first
    const uint4* table;         // 2 * kept entries
    float4* out;                // the size^2 level, [6][size][size]
    int kept, per_slice;        // per_slice = ceil(kept / S)
    float wsum;
    int size, face0, y0, rows, texels;    // texels = faces * rows * size of this dispatch
};

template <int S>
__global__ __launch_bounds__(S > 1 ? 64 * S : 256) void k_prefilter_ggx(GgxParams p) {
    __shared__ float part[S > 1 ? S - 1 : 1][3][64];
    const int lane = threadIdx.x & 63;
    const int slice = S > 1 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
    const int ti = S > 1 ? blockIdx.x * 64 + lane : blockIdx.x * 256 + threadIdx.x;     // S == 1: four waves, four times 64 texels
    const bool live = ti < p.texels;
    const int tc = live ? ti : p.texels - 1;                       // idle lanes shadow the last texel: every address stays inside
    const int x = tc % p.size, fy = tc / p.size;
    const int y = p.y0 + fy % p.rows, face = p.face0 + fy / p.rows;

    float nrm[3], T[3], B[3];
    pggx_texel_dir(face, x, y, p.size, nrm);
    pggx_frame(nrm, T, B);

    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    const int i0 = slice * p.per_slice, i1 = min(p.kept, i0 + p.per_slice);
    for (int i = i0; i < i1; ++i) {
        const uint4 e0 = p.table[2 * i], e1 = p.table[2 * i + 1];
        const float lx = __uint_as_float(e0.x), ly = __uint_as_float(e0.y), lz = __uint_as_float(e0.z), f = __uint_as_float(e0.w);
        float d[3];
        pggx_sample_dir(nrm, T, B, lx, ly, lz, d);
        const CubeST cs = cube_select(mk3(d[0], d[1], d[2]));
        float s, t;
        cube_st_exact(cs, &s, &t);
        const int n0 = (int)e1.y, n1 = (int)e1.w;
        const float4* lvl0 = p.src + e1.x;
        const f3 c0 = fetch_rgb_tap(lvl0, n0, cube_tap_from_st(cs.face, s, t, n0));
        f3 c1 = c0;
        if (e1.z != e1.x) c1 = fetch_rgb_tap(p.src + e1.z, n1, cube_tap_from_st(cs.face, s, t, n1));
        ar = fmaf(lz, lerp_fma(c0.x, c1.x, f), ar);
        ag = fmaf(lz, lerp_fma(c0.y, c1.y, f), ag);
        ab = fmaf(lz, lerp_fma(c0.z, c1.z, f), ab);
    }
    if (S > 1) {
        if (slice > 0) { part[slice - 1][0][lane] = ar; part[slice - 1][1][lane] = ag; part[slice - 1][2][lane] = ab; }
        __syncthreads();
        if (slice > 0) return;
        for (int k = 0; k < S - 1; ++k) { ar += part[k][0][lane]; ag += part[k][1][lane]; ab += part[k][2][lane]; }
    }
    if (live) p.out[((size_t)face * p.size + y) * p.size + x] = make_float4(ar / p.wsum, ag / p.wsum, ab / p.wsum, 1.0f);
}

extern "C" int pbrk_prefilter_ggx(const void* src_bordered, const void* table, int kept, float wsum, void* out, int out_size,
                                  int face0, int face1, int y0, int y1, void* stream) {
    if (!src_bordered || !table || !out || kept < 0 || kept > PGGX_MAX_SAMPLES || out_size < 1 || out_size > 16384) return PBRK_E_ARG;
    if (face0 < 0 || face1 > 6 || face0 >= face1 || y0 < 0 || y1 > out_size || y0 >= y1) return PBRK_E_ARG;
    const int S = pggx_slices(out_size);
    GgxParams p;
    p.src = (const float4*)src_bordered; p.table = (const uint4*)table; p.out = (float4*)out;
    p.kept = kept; p.per_slice = (kept + S - 1) / S; p.wsum = wsum;
    p.size = out_size; p.face0 = face0; p.y0 = y0; p.rows = y1 - y0;
    const long long texels = (long long)(face1 - face0) * (y1 - y0) * out_size;      // <= 6 * 16384^2 < 2^31
    p.texels = (int)texels;
    const int per_block = S > 1 ? 64 : 256;
    const dim3 grid((unsigned)((texels + per_block - 1) / per_block));
    hipStream_t st = (hipStream_t)stream;
    if (S == 1) hipLaunchKernelGGL(k_prefilter_ggx<1>, grid, dim3(256), 0, st, p);
    else if (S == 4) hipLaunchKernelGGL(k_prefilter_ggx<4>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_prefilter_ggx<16>, grid, dim3(1024), 0, st, p);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}
