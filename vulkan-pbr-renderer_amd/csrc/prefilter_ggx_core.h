// prefilter_ggx_core.h -- the contract of K21 (DESIGN.md "K21"): the specular cube prefiltered by GGX importance sampling with
// filtered source lookups (Krivanek-Colbert, Karis), written once for the device kernel of k_prefilter_ggx.hip, for the host code of
// gpu_hip.cpp that builds the op's sample table and answers GPUX_PrefilterGGXSamples, and for the host test program.
//
// Sample table (host only, double, the same for every texel).  a = r^2; for i = 0 .. N-1:
//   xi1 = (i + 1/2) / N, xi2 = the 32-bit base-2 radical inverse of i, phi = 2 pi xi2
//   cos^2 t = (1 - xi1) / (1 + (a^2 - 1) xi1)                                   the GGX half vector for V = N = (0, 0, 1)
//   l = (2 cos t sin t cos phi, 2 cos t sin t sin phi, 2 cos^2 t - 1)            the light direction, reflect(-V, h)
//   D = a^2 / (pi (cos^2 t (a^2 - 1) + 1)^2), pdf(l) = D / 4                     (N.H = V.H)
//   lod = clamp(1/2 log2(6 n0^2 / (4 pi N pdf)) + lod_bias, 0, levels - 1)      the level whose texel solid angle is the sample's
// An entry is {l.x, l.y, l.z, lod}, each rounded once to fp32; entries whose fp32 l.z is not positive are dropped, the rest keep the
// order of i.  wsum = the double sum of the kept fp32 l.z, rounded once to fp32.
//
// Texel (face, x, y) of a size^2 level, in fp32, every operation separately rounded (-ffp-contract=off, correctly rounded / and
// sqrt), FMAs only where written:
//   Nrm = pggx_texel_dir: face_texel_dir of pbr_device.h (an IEEE quotient by n is the product by 1/n it forms for powers of two)
//   up = |Nrm.z| < 0.999f ? (0, 0, 1) : (1, 0, 0);  T = normalize(cross(up, Nrm));  B = cross(Nrm, T)
//   per entry: d = fmaf(Nrm, l.z, fmaf(B, l.y, T * l.x));  l0 = floorf(lod), f = lod - floorf(lod), l1 = min(l0 + 1, levels - 1)
//              c = lerp_fma(c0, c1, f), c0 / c1 = cube_fetch_rgba<true> of the bordered levels l0 / l1;  acc = fmaf(l.z, c, acc)
//   out.rgb = acc / wsum, out.a = 1.  The order of accumulation is free but fixed for a given (size, kept count).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PGGX_FN __host__ __device__ __forceinline__
#else
#define PGGX_FN static inline
#endif

#define PGGX_PI 3.14159265358979323846
#define PGGX_MAX_SAMPLES 4096
#define PGGX_MAX_LEVELS 16

// ---- the table: host only ----
static inline double pggx_radical_inverse(uint32_t i) {
    i = (i << 16) | (i >> 16);
    i = ((i & 0x55555555u) << 1) | ((i & 0xAAAAAAAAu) >> 1);
    i = ((i & 0x33333333u) << 2) | ((i & 0xCCCCCCCCu) >> 2);
    i = ((i & 0x0F0F0F0Fu) << 4) | ((i & 0xF0F0F0F0u) >> 4);
    i = ((i & 0x00FF00FFu) << 8) | ((i & 0xFF00FF00u) >> 8);
    return (double)i * (1.0 / 4294967296.0);
}
// The kept entries {l.x, l.y, l.z, lod} into xyz_lod (room for 4 * sample_count floats) -> their number; *wsum as above.
// The caller has checked: roughness in (0, 1], sample_count in 1 .. PGGX_MAX_SAMPLES, src_size >= 1, src_levels >= 1, finite lod_bias.
static inline uint32_t pggx_fill_table(float roughness, uint32_t sample_count, uint32_t src_size, uint32_t src_levels, float lod_bias,
                                       float* xyz_lod, float* wsum) {
    const double a = (double)roughness * (double)roughness, a2 = a * a;
    const double texels = 6.0 * (double)src_size * (double)src_size, top = (double)(src_levels - 1);
    uint32_t kept = 0;
    double sum = 0.0;
    for (uint32_t i = 0; i < sample_count; ++i) {
        const double xi1 = ((double)i + 0.5) / (double)sample_count, phi = 2.0 * PGGX_PI * pggx_radical_inverse(i);
        const double c2 = (1.0 - xi1) / (1.0 + (a2 - 1.0) * xi1);
        const double ct = sqrt(c2), st = sqrt(1.0 - c2);
        const float z = (float)(2.0 * c2 - 1.0);
        if (!(z > 0.0f)) continue;
        const double den = c2 * (a2 - 1.0) + 1.0;
        const double pdf = a2 / (PGGX_PI * den * den) / 4.0;
        double lod = 0.5 * log2(texels / (4.0 * PGGX_PI * (double)sample_count * pdf)) + (double)lod_bias;
        lod = lod < 0.0 ? 0.0 : (lod > top ? top : lod);
        float* e = xyz_lod + 4 * (size_t)kept++;
        e[0] = (float)(2.0 * ct * st * cos(phi)); e[1] = (float)(2.0 * ct * st * sin(phi)); e[2] = z; e[3] = (float)lod;
        sum += (double)z;
    }
    *wsum = (float)sum;
    return kept;
}

// ---- the frame of a texel and the direction of a sample: host and device ----
PGGX_FN void pggx_normalize(const float a[3], float r[3]) {
    const float len = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    r[0] = a[0] / len; r[1] = a[1] / len; r[2] = a[2] / len;
}
PGGX_FN void pggx_cross(const float a[3], const float b[3], float r[3]) {
    r[0] = a[1] * b[2] - b[1] * a[2]; r[1] = a[2] * b[0] - b[2] * a[0]; r[2] = a[0] * b[1] - b[0] * a[1];
}
PGGX_FN void pggx_texel_dir(int face, int ix, int iy, int n, float nrm[3]) {
    const float u = ((float)ix + 0.5f) / (float)n, v = ((float)iy + 0.5f) / (float)n;
    const float sc = 2 * (u - 0.5f), tc = 2 * (v - 0.5f);
    float r[3];
    switch (face) {
    case 0: r[0] = 1.0f; r[1] = -tc; r[2] = -sc; break;
    case 1: r[0] = -1.0f; r[1] = -tc; r[2] = sc; break;
    case 2: r[0] = sc; r[1] = 1.0f; r[2] = tc; break;
    case 3: r[0] = sc; r[1] = -1.0f; r[2] = -tc; break;
    case 4: r[0] = sc; r[1] = -tc; r[2] = 1.0f; break;
    default: r[0] = -sc; r[1] = -tc; r[2] = -1.0f; break;
    }
    pggx_normalize(r, nrm);
}
PGGX_FN void pggx_frame(const float nrm[3], float t[3], float b[3]) {
    const bool z_up = fabsf(nrm[2]) < 0.999f;
    const float up[3] = {z_up ? 0.0f : 1.0f, 0.0f, z_up ? 1.0f : 0.0f};
    float c[3];
    pggx_cross(up, nrm, c);
    pggx_normalize(c, t);
    pggx_cross(nrm, t, b);
}
PGGX_FN void pggx_sample_dir(const float nrm[3], const float t[3], const float b[3], float lx, float ly, float lz, float d[3]) {
    for (int k = 0; k < 3; ++k) d[k] = fmaf(nrm[k], lz, fmaf(b[k], ly, t[k] * lx));
}

// ---- how a level's samples are split: a function of the level's size alone, so that a texel's bytes do not depend on the faces
//      and rows it was dispatched with.  S waves of a workgroup share 64 texels; wave k takes entries [k q, (k + 1) q), q = ceil(K / S)
//      (possibly none), and the partial sums are added in the order of k. ----
PGGX_FN int pggx_slices(int size) { return size >= 128 ? 1 : size >= 64 ? 4 : 16; }
