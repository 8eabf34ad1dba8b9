// brdf_lut_ggx_core.h -- the contract of K22 (DESIGN.md "K22"): the split-sum BRDF LUT by GGX importance sampling (Karis'
// IntegrateBRDF), the other half of K21's pair, written once for the device kernel of k_lut_ggx.hip, for the host code of gpu_hip.cpp
// that builds the op's sample table and answers GPUX_BrdfLutGGXSamples, and for the host test program.
//
// Texel (x, y) of a w x h map, in fp32: nv = (x + 1/2) / w (N.V), r = (y + 1/2) / h (roughness); K1's parametrisation.
//
// Sample table (host only, double, the same for every texel).  For i = 0 .. N-1:
//   xi1 = (i + 1/2) / N, phi = 2 pi (the 32-bit base-2 radical inverse of i); the entry is {xi1, cos phi, sin phi}, each rounded once
//   to fp32.  sin phi is part of the table and of no value below: V.y = 0, so H.y = sin t sin phi enters neither V.H nor L.z.
//
// Everything else in fp32, every operation separately rounded (-ffp-contract=off, correctly rounded / and sqrt), fmaf only where
// written.  N = (0, 0, 1), so N.H = H.z and N.L = L.z.
//   per row:            a = r * r;  a2 = a * a
//   per (row, sample):  c2 = (1 - xi1) / (1 + (a2 - 1) * xi1)                    cos^2 of the GGX half vector's polar angle
//                       hz = sqrtf(c2);  hx = sqrtf(1 - c2) * cos phi;  hz2 = hz + hz;  rhz = 1 / hz
//   per texel:          vx = sqrtf(1 - nv * nv)                                  V = (vx, 0, nv)
//     Smith-Schlick:    k = a * 0.5f;  omk = 1 - k;  cv = 1 / fmaf(nv, omk, k)   G1(nv) / nv, G1(c) = c / (c (1 - k) + k)
//     Smith correlated: oma2 = 1 - a2;  sv = sqrtf(fmaf(nv * nv, oma2, a2))
//   per (texel, sample):
//     vh = fmaf(vx, hx, nv * hz)                                                 V.H
//     lz = fmaf(vh, hz2, -nv)                                                    L.z = 2 (V.H) H.z - V.z
//     live = lz > 0 && vh > 0
//     q = fmaxf(1 - vh, 0);  q2 = q * q;  fc = (q2 * q2) * q                     (1 - V.H)^5; the maximum keeps fc >= 0 where vh rounds past 1
//     num = (vh * rhz) * lz
//     Smith-Schlick:    gv = (num * cv) / fmaf(lz, omk, k)                       G (V.H) / (N.H N.V), G = G1(nv) G1(lz)
//     Smith correlated: gv = (num + num) / fmaf(lz, sv, nv * sqrtf(fmaf(lz * lz, oma2, a2)))
//                                                                                4 Vis (V.H) (N.L) / (N.H), Vis = 1/2 / (lz sv + nv sl)
//     gv = 0 where not live (a selection, not a product: the quotient of a dead sample may be anything)
//     tA = gv * (1 - fc);  tB = gv * fc                                          the per-sample terms, both >= 0
//   texel: A = (sum tA) / (float)N, B = (sum tB) / (float)N.  The order of accumulation is free (the kernel's is a chain of
//   acc = fmaf(gv, 1 - fc, acc) per run of samples, blg_slices runs per texel added in their order) but fixed for a given (w, h, N).
//
// Every denominator is positive, so no texel is NaN or infinite:
//   xi1 <= 1 - 1/(2N) < 1 in fp32 (N <= 4096), a2 - 1 >= -1, and rounding is monotone: 1 + (a2 - 1) xi1 >= 1 - xi1 >= 2^-13, hence
//   0 < c2 <= 1, hz > 0, rhz finite and 1 - c2 >= 0.  nv = (x + 1/2) / w lies in [1/(2w), 1 - 1/(2w)], so vx is real and nv > 0.
//   r >= 1/(2h) >= 2^-13: a >= 2^-26 and a2 >= 2^-52 are normal numbers.  k = a/2 > 0 and omk = 1 - k in [1/2, 1]: fmaf(nv, omk, k) >= k
//   and, for a live sample, fmaf(lz, omk, k) >= k.  oma2 in [0, 1]: both radicands are >= a2 > 0, sv > 0, and with lz > 0 and nv > 0
//   the correlated denominator is > 0.  vh <= 1 + a few ulp and lz <= 1 + a few ulp bound every numerator.
#pragma once
#include <math.h>
#include <stdint.h>

#include "prefilter_ggx_core.h"          /* pggx_radical_inverse, PGGX_PI */

#if defined(__HIPCC__)
#define BLG_FN __host__ __device__ __forceinline__
#else
#define BLG_FN static inline
#endif

#define BLG_MAX_SAMPLES 4096
#define BLG_MAX_EXTENT 4096
#define BLG_SMITH_SCHLICK 0              /* GPUX_BrdfLut_SmithSchlick */
#define BLG_SMITH_CORRELATED 1           /* GPUX_BrdfLut_SmithCorrelated */

// ---- the table: host only.  {xi1, cos phi, sin phi} per sample into xi_cos_sin (room for 3 * sample_count floats) ----
static inline void blg_fill_table(uint32_t sample_count, float* xi_cos_sin) {
    for (uint32_t i = 0; i < sample_count; ++i) {
        const double phi = 2.0 * PGGX_PI * pggx_radical_inverse(i);
        float* e = xi_cos_sin + 3 * (size_t)i;
        e[0] = (float)(((double)i + 0.5) / (double)sample_count); e[1] = (float)cos(phi); e[2] = (float)sin(phi);
    }
}

// ---- host and device ----
typedef struct BlgHalf { float hx, hz, hz2, rhz; } BlgHalf;          // per (row, sample)
typedef struct BlgView { float nv, vx, c0, c1, c2; } BlgView;        // per texel: Schlick {cv, omk, k}, correlated {sv, oma2, a2}

BLG_FN float blg_coord(int i, int n) { return ((float)i + 0.5f) / (float)n; }

BLG_FN BlgHalf blg_half(float a2, float xi1, float cos_phi) {
    const float c2 = (1.0f - xi1) / (1.0f + (a2 - 1.0f) * xi1);
    BlgHalf h;
    h.hz = sqrtf(c2); h.hx = sqrtf(1.0f - c2) * cos_phi; h.hz2 = h.hz + h.hz; h.rhz = 1.0f / h.hz;
    return h;
}

BLG_FN BlgView blg_view(int visibility, float nv, float a, float a2) {
    BlgView v;
    v.nv = nv; v.vx = sqrtf(1.0f - nv * nv);
    if (visibility == BLG_SMITH_SCHLICK) { v.c2 = a * 0.5f; v.c1 = 1.0f - v.c2; v.c0 = 1.0f / fmaf(nv, v.c1, v.c2); }
    else { v.c2 = a2; v.c1 = 1.0f - a2; v.c0 = sqrtf(fmaf(nv * nv, v.c1, a2)); }
    return v;
}

// gv (0 where the sample is not live), 1 - fc and fc of one sample: tA = gv * omfc, tB = gv * fc
BLG_FN void blg_sample(int visibility, BlgView v, BlgHalf h, float* gv, float* omfc, float* fc) {
    const float vh = fmaf(v.vx, h.hx, v.nv * h.hz);
    const float lz = fmaf(vh, h.hz2, -v.nv);
    const float q = fmaxf(1.0f - vh, 0.0f), q2 = q * q, f = (q2 * q2) * q;
    const float num = (vh * h.rhz) * lz;
    float g;
    if (visibility == BLG_SMITH_SCHLICK) g = (num * v.c0) / fmaf(lz, v.c1, v.c2);
    else g = (num + num) / fmaf(lz, v.c0, v.nv * sqrtf(fmaf(lz * lz, v.c1, v.c2)));
    *gv = (lz > 0.0f && vh > 0.0f) ? g : 0.0f;
    *omfc = 1.0f - f; *fc = f;
}

// ---- how a row's samples are split: a function of the width alone, so that a texel's bytes do not depend on the rows it was
//      dispatched with.  The 16 waves of a row's workgroup share its ceil(w / 64) groups of 64 columns: S waves per group, wave k of a
//      group takes samples [k q, (k + 1) q), q = ceil(N / S) (possibly none), and the partial sums are added in the order of k. ----
BLG_FN int blg_slices(int w) {
    const int groups = (w + 63) / 64;
    return groups >= 9 ? 1 : groups >= 5 ? 2 : groups >= 3 ? 4 : groups == 2 ? 8 : 16;
}
