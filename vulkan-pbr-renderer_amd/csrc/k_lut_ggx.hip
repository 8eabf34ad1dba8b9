// k_lut_ggx.hip -- K22 (an extension: the reference's live LUT is K1's Beckmann quadrature): the split-sum BRDF LUT by
// GGX importance sampling, rows [y0, y1) of a w x h map.  The contract is in brdf_lut_ggx_core.h.
//
// One workgroup of 16 waves per row.  The half vector of a sample depends on (row, sample) only, the view vector on the column only:
// the workgroup first builds its row's table {hx, hz, 2 hz, 1 / hz} in LDS (16 bytes per sample, 64 KB at the cap of 4096: the
// division and the two square roots of a sample are done once per row, not once per lane), then lanes own columns and the sample
// index is wave-uniform, so every entry arrives as one broadcast 16-byte LDS read.  Per sample a lane does V.H, L.z, the Fresnel
// power, one division (plus one square root for the correlated term) and two FMAs.
//
// Narrow maps do not fill 16 waves with columns: blg_slices(w) waves share a group of 64 columns, wave k of a group takes a
// contiguous run of the samples, the partial sums go through LDS (the table's own storage, free by then) and wave 0 of the group adds
// them in the order of k: no atomics, the same bytes every time, whatever rows the texel was dispatched with.  Maps of 9 groups and
// more (w > 512) run one wave per group and walk the groups.
#include "pbr_device.h"
#include "pbr_kernels.h"
#include "brdf_lut_ggx_core.h"
#include <hip/hip_fp16.h>

#define BLG_WAVES 16

struct LutGgxParams {
    void* out;                  // the whole map, [h][w] texels of fmt
    const float* table;         // {xi1, cos phi, sin phi} per sample
    int fmt, w, h, n, y0;
    int slices, per_slice;      // blg_slices(w); ceil(n / slices)
};

__device__ __forceinline__ void lut_ggx_store(const LutGgxParams& p, int x, int y, float A, float B) {
    const size_t o = (size_t)y * p.w + x;
    if (p.fmt == PBRK_FMT_RG16F) ((__half2*)p.out)[o] = __halves2half2(__float2half_rn(A), __float2half_rn(B));
    else if (p.fmt == PBRK_FMT_RG32F) ((float2*)p.out)[o] = make_float2(A, B);
    else ((float4*)p.out)[o] = make_float4(A, B, 0.0f, 1.0f);
}

template <int VIS>
__global__ __launch_bounds__(64 * BLG_WAVES) void k_brdf_lut_ggx(LutGgxParams p) {
    __shared__ __attribute__((aligned(16))) float4 tab[BLG_MAX_SAMPLES];
    const int y = p.y0 + (int)blockIdx.x;
    const float r = blg_coord(y, p.h), a = r * r, a2 = a * a;
    for (int i = threadIdx.x; i < p.n; i += 64 * BLG_WAVES) {
        const BlgHalf hv = blg_half(a2, p.table[3 * i], p.table[3 * i + 1]);
        tab[i] = make_float4(hv.hx, hv.hz, hv.hz2, hv.rhz);
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int S = p.slices, groups = (p.w + 63) >> 6;
    const int slice = wave % S;
    const int i0 = min(p.n, slice * p.per_slice), i1 = min(p.n, i0 + p.per_slice);
    const float nf = (float)p.n;
    float sa = 0.0f, sb = 0.0f;
    // S == 1: the wave walks the groups wave, wave + 16, ...; S > 1: S * groups <= 16, so the step ends the loop after the wave's one group
    for (int cg = wave / S; cg < groups; cg += BLG_WAVES / S) {
        const int x = cg * 64 + lane;
        const BlgView v = blg_view(VIS, blg_coord(min(x, p.w - 1), p.w), a, a2);     // idle lanes shadow the last column
        sa = 0.0f; sb = 0.0f;
        for (int i = i0; i < i1; ++i) {
            const float4 e = tab[i];
            BlgHalf hv; hv.hx = e.x; hv.hz = e.y; hv.hz2 = e.z; hv.rhz = e.w;
            float gv, omfc, fc;
            blg_sample(VIS, v, hv, &gv, &omfc, &fc);
            sa = fmaf(gv, omfc, sa);
            sb = fmaf(gv, fc, sb);
        }
        if (S == 1 && x < p.w) lut_ggx_store(p, x, y, sa / nf, sb / nf);
    }
    if (S == 1) return;                                      // uniform over the workgroup

    const bool mine = wave / S < groups;                     // the wave holds a share of a group's sums
    const int x = (wave / S) * 64 + lane;
    __syncthreads();                                         // every wave is done with the table: its storage takes the partial sums
    float* part = (float*)tab;                               // [wave][2][64], 8 KB
    if (mine && slice > 0) { part[(wave * 2 + 0) * 64 + lane] = sa; part[(wave * 2 + 1) * 64 + lane] = sb; }
    __syncthreads();
    if (!mine || slice > 0) return;
    for (int k = 1; k < S; ++k) { sa += part[((wave + k) * 2 + 0) * 64 + lane]; sb += part[((wave + k) * 2 + 1) * 64 + lane]; }
    if (x < p.w) lut_ggx_store(p, x, y, sa / nf, sb / nf);
}

extern "C" int pbrk_brdf_lut_ggx(void* out, int out_format, int w, int h, int nsamples, int visibility, const void* table,
                                 int y0, int y1, void* stream) {
    if (!out || !table || w < 1 || w > BLG_MAX_EXTENT || h < 1 || h > BLG_MAX_EXTENT || nsamples < 1 || nsamples > BLG_MAX_SAMPLES) return PBRK_E_ARG;
    if (visibility != BLG_SMITH_SCHLICK && visibility != BLG_SMITH_CORRELATED) return PBRK_E_ARG;
    if (y0 < 0 || y1 > h || y0 >= y1) return PBRK_E_ARG;
    if (out_format != PBRK_FMT_RG16F && out_format != PBRK_FMT_RG32F && out_format != PBRK_FMT_RGBA32F) return PBRK_E_FORMAT;
    LutGgxParams p;
    p.out = out; p.table = (const float*)table; p.fmt = out_format; p.w = w; p.h = h; p.n = nsamples; p.y0 = y0;
    p.slices = blg_slices(w); p.per_slice = (nsamples + p.slices - 1) / p.slices;
    const dim3 grid((unsigned)(y1 - y0)), block(64 * BLG_WAVES);
    hipStream_t st = (hipStream_t)stream;
    if (visibility == BLG_SMITH_SCHLICK) hipLaunchKernelGGL(k_brdf_lut_ggx<BLG_SMITH_SCHLICK>, grid, block, 0, st, p);
    else hipLaunchKernelGGL(k_brdf_lut_ggx<BLG_SMITH_CORRELATED>, grid, block, 0, st, p);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}
