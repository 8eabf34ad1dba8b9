// sh_shade_core.h -- the SH9 ambient term of the shade pass (K5 with PBRK_SHADE_SH9, DESIGN.md 4 "K5, SH9 ambient"): the irradiance of
// sh_core.h's sh_irradiance evaluated per pixel from 27 folded fp32 constants instead of a lookup in the irradiance cube.  Written once
// for the kernels of k_shade.hip / k_shade_fast.hip and for a host compiler (tests/sh_shade_core_host.cpp).
//
// Fold (once per workgroup, not per pixel):  k[3 i + c] = (float)((a_i K_i) * coef[3 i + c]),  a_i the irradiance weights of
// sh_irradiance, K_i the basis constants of sh_basis, so that Y_i = K_i p_i with p = {1, y, z, x, xy, yz, 3 z^2 - 1, xz, x^2 - y^2}.
// The nine products a_i K_i are the double literals below (tests/test_sh_shade_cpu.py holds them to sh_core.h's expressions bit for
// bit); the product with the coefficient is one double multiplication, rounded once to fp32.
//
// Evaluation for a RAW normal n = (x, y, z) of any non-zero length (the shader never normalises N, lighting_pass.glsl:433-442, and a
// cube lookup does not care): with r2 = |n|^2, s = 1 / sqrt(r2), s2 = 1 / r2 the homogeneous form
//   E_c = k0 + s (k1 y + k2 z + k3 x) + s2 (k4 xy + k5 yz + k6 (3 z^2 - r2) + k7 xz + k8 (x^2 - y^2))
// in fp32, in ONE operation order with explicit fmaf (below).  3 z^2 - r2 is formed as 2 z^2 - (x^2 + y^2): 2 z is exact.  No clamp:
// like K17's map the series may ring negative; the shader's final max(out, 0) (:712) is what applies.
//
// Error of that order against sh_irradiance in double, u = 2^-24, per unit of |k_i| (normalised n; |p_i| <= 1, 1, 1, 1/2, 1/2, 2, 1/2, 1):
//   fold 1 rounding of k_i; r2 three roundings (<= 3 u r2); s and s2 one reciprocal (square root) of at most 1 ulp = 2 u each on top of
//   r2's error: s within 3.5 u, s2 within 5 u; the products xy, yz, xz one rounding; q6 = 2 z^2 - (x^2 + y^2) within 4 u r2, q8 within
//   2 u r2; band 1 is a chain of 3 roundings, band 2 a chain of 5 in which k6 q6 -- the largest term -- is added LAST (1 rounding),
//   k8 q8 before it (2), then k4 xy (3), k5 yz (4), k7 xz (5); two final fmaf, each a rounding of at most the whole sum.
//   k0: 3 u;  k1..k3: 1 + 3 + 3.5 + 2 = 9.5 u;  k4, k5, k7: at most 7 u;  k8: 1 + 2 + 2 + 5 + 2 = 12 u;  k6: 2 + 4 + 2 + 10 + 4 = 22 u.
//   Hence |E32 - E64| <= 22 * 2^-24 * sum_i |k[3 i + c]| = 1.32e-6 sum |k|, inside the 2e-6 sum |k| that the tests hold it to.
// The host build takes 1 / sqrtf and 1 / r2 (correctly rounded: inside the 1-ulp allowance); the device takes v_rsq_f32 / v_rcp_f32.
#pragma once
#include "sh_core.h"

// a_i K_i, i = 0 .. 8: 1/2 sqrt(1/4pi); 1/3 sqrt(3/4pi) x 3; 1/8 sqrt(15/4pi) x 2; 1/8 sqrt(5/16pi); 1/8 sqrt(15/4pi); 1/8 sqrt(15/16pi)
SH_FN double sh_shade_weight(int i) {
    switch (i) {
    case 0: return 0x1.20dd750429b6dp-3;
    case 1: case 2: case 3: return 0x1.4d8d7a58fa311p-3;
    case 6: return 0x1.42f601a8c679bp-5;
    case 8: return 0x1.17b14102b0694p-4;
    default: return 0x1.17b14102b0694p-3;
    }
}
// one folded constant: entry j = 3 i + c of k
SH_FN float sh_shade_fold_one(double coef_j, int j) { return (float)(sh_shade_weight(j / 3) * coef_j); }
SH_FN void sh_shade_fold(const double coef[27], float k[27]) {
    for (int j = 0; j < 27; ++j) k[j] = sh_shade_fold_one(coef[j], j);
}

SH_FN float sh_shade_rsqrt(float r2) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rsqf(r2);
#else
    return 1.0f / sqrtf(r2);
#endif
}
SH_FN float sh_shade_rcp(float r2) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(r2);
#else
    return 1.0f / r2;
#endif
}

// E / (2 pi) of the folded constants k (index 3 i + c) for the raw normal (x, y, z), not clamped
SH_FN void sh_shade_eval(const float k[27], float x, float y, float z, float rgb[3]) {
    const float r2 = fmaf(x, x, fmaf(y, y, z * z));
    const float s = sh_shade_rsqrt(r2), s2 = sh_shade_rcp(r2);
    const float xy = x * y, yz = y * z, xz = x * z;
    const float q6 = fmaf(2.0f * z, z, -fmaf(x, x, y * y));
    const float q8 = fmaf(x, x, -(y * y));
    for (int c = 0; c < 3; ++c) {
        const float l1 = fmaf(k[3 + c], y, fmaf(k[6 + c], z, k[9 + c] * x));
        const float l2 = fmaf(k[18 + c], q6, fmaf(k[24 + c], q8, fmaf(k[12 + c], xy, fmaf(k[15 + c], yz, k[21 + c] * xz))));
        rgb[c] = fmaf(s2, l2, fmaf(s, l1, k[c]));
    }
}
