// shadow_core.h -- the sampler2DShadow tap shared by K5 (k_shade.hip) and K14 (voxelize_core.h); also compiles for a host compiler.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SHADOW_FN __host__ __device__ __forceinline__
#else
#define SHADOW_FN static inline
#endif

SHADOW_FN int shadow_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sampler2DShadow + SAMPLER_PERCENTAGE_CLOSER (render.cpp:664-673: linear, clamp, compare Less): each bilinear tap contributes
// (ref < texel ? 1 : 0); coordinates snapped to 1/256 texel (the 2-D sampler convention of k_post.hip / the oracle).  EXACT.
SHADOW_FN float shadow_sample(const float* __restrict__ d, int w, int h, float u, float v, float ref) {
    float fx = u * (float)w - 0.5f, fy = v * (float)h - 0.5f;
    fx = floorf(fx * 256.0f + 0.5f) * (1.0f / 256.0f);
    fy = floorf(fy * 256.0f + 0.5f) * (1.0f / 256.0f);
    float flx = floorf(fx), fly = floorf(fy);
    float a = fx - flx, b = fy - fly;
    int i0 = (int)fminf(fmaxf(flx, -1.0f), (float)w), j0 = (int)fminf(fmaxf(fly, -1.0f), (float)h);   // float-domain clamp: see snap_split
    int i1 = shadow_clampi(i0 + 1, 0, w - 1), j1 = shadow_clampi(j0 + 1, 0, h - 1);
    i0 = shadow_clampi(i0, 0, w - 1); j0 = shadow_clampi(j0, 0, h - 1);
    float c00 = ref < d[j0 * w + i0] ? 1.0f : 0.0f, c10 = ref < d[j0 * w + i1] ? 1.0f : 0.0f;
    float c01 = ref < d[j1 * w + i0] ? 1.0f : 0.0f, c11 = ref < d[j1 * w + i1] ? 1.0f : 0.0f;
    float top = c00 + a * (c10 - c00), bot = c01 + a * (c11 - c01);
    return top + b * (bot - top);
}
