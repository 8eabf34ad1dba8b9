// gridview_core.h -- the light-grid visualiser of the lighting pass (K16), written once for the device kernel of
// k_gridview.hip and for a host compiler: plain scalar C++ in the shader's operation order, separately rounded fp32 (no FMA
// contraction, correctly rounded / and sqrt), so a CPU build evaluates the contract exactly as the kernel does.
// Cited shader lines: lighting_pass.glsl of the reference renderer, the "VOXEL DEBUG RAY TRACER" block :463-491.
//
// The block replaces the shading of every pixel, sky included: a ray from the pixel's point on the near plane marches through
// LIGHTGRID in up to GV_MAX_STEPS half-voxel steps; the first trilinear sample with alpha > 0.3 gives the colour, whose luminance is
// remapped by its square root.  The sampler clamps, so a ray outside the cube keeps reading edge voxels and can still hit.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GV_FN __host__ __device__ __forceinline__
#else
#define GV_FN static inline
#endif

#define GV_MAX_STEPS 512                                                       // :474

struct GvRay { float ro[3], rd[3]; };

GV_FN float gv_fract(float x) { return x - floorf(x); }
// InterleavedGradientNoise (:119-121) and noise_1 (:456-457), as K5 computes them
GV_FN float gv_ign(float px, float py) { return gv_fract(52.9829189f * gv_fract(0.06711056f * px + 0.00583715f * py)); }
GV_FN float gv_noise_1(float frag_x, float frag_y, float frame_idx_mod_59) {
    const float noise_offset = (1000 * 1.61803398875f) * frame_idx_mod_59;
    return gv_fract(gv_ign(frag_x, frag_y) + noise_offset);
}

// :465-470.  wfc = world_space_from_clip (column major), cam = camera_pos, (u, v) = fs_uv, (frag_x, frag_y) = gl_FragCoord.xy
GV_FN void gv_ray(const float* wfc, const float* cam, float lightgrid_scale, float frame_idx_mod_59, float u, float v,
                  float frag_x, float frag_y, GvRay& r) {
    const float cx = u * 2.0f - 1.0f, cy = v * 2.0f - 1.0f;
    float near_p[4];
    for (int k = 0; k < 4; ++k) near_p[k] = ((wfc[k] * cx + wfc[4 + k] * cy) + wfc[8 + k] * 0.0f) + wfc[12 + k] * 1.0f;
    const float w = near_p[3];
    for (int k = 0; k < 4; ++k) near_p[k] = near_p[k] / w;
    float d[3];
    for (int k = 0; k < 3; ++k) { r.ro[k] = near_p[k] * lightgrid_scale; d[k] = near_p[k] - cam[k]; }
    const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);          // normalize(a) = a / sqrt(dot(a, a))
    for (int k = 0; k < 3; ++k) r.rd[k] = (d[k] / len) * (1.0f / 128.0f);
    const float noise_1 = gv_noise_1(frag_x, frag_y, frame_idx_mod_59);
    for (int k = 0; k < 3; ++k) r.ro[k] = r.ro[k] + noise_1 * r.rd[k];
}

// one march step (:475-476): ro += rd, never ro0 + i * rd; p = the texture coordinate of the sample
GV_FN void gv_step(GvRay& r, float p[3]) {
    for (int k = 0; k < 3; ++k) { r.ro[k] = r.ro[k] + r.rd[k]; p[k] = r.ro[k] * 0.5f + 0.5f; }
}
GV_FN bool gv_hits(float alpha) { return alpha > 0.3f; }                       // :479

// :473, :480-489 from the march's outcome: rgb = the colour of the sample that hit (ignored without a hit)
GV_FN void gv_resolve(bool hit, const float* rgb, float out[4]) {
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.00001f};
    if (hit) { sum[0] = 10.0f * rgb[0]; sum[1] = 10.0f * rgb[1]; sum[2] = 10.0f * rgb[2]; sum[3] = 10.0f * 1.0f; }
    const float w = sum[3];
    for (int k = 0; k < 4; ++k) sum[k] = sum[k] / w;                           // not a no-op: 10 x / 10 rounds twice
    const float luminance = 0.299f * sum[0] + 0.587f * sum[1] + 0.114f * sum[2];
    const float s = sqrtf(luminance) / fmaxf(luminance, 0.0001f);
    out[0] = sum[0] * s; out[1] = sum[1] * s; out[2] = sum[2] * s; out[3] = 1.0f;
}

// The whole block for one pixel.  sample(p, rgba) is texture(sampler3D(LIGHTGRID, SAMPLER_LINEAR_CLAMP), p).  Returns the step
// (0 .. GV_MAX_STEPS - 1) of the sample that hit, -1 without a hit; hit_ro (may be NULL) receives ro at that sample.
template <class Sampler>
GV_FN int gv_pixel(const float* wfc, const float* cam, float lightgrid_scale, float frame_idx_mod_59, float u, float v,
                   float frag_x, float frag_y, const Sampler& sample, float out[4], float* hit_ro) {
    GvRay r;
    gv_ray(wfc, cam, lightgrid_scale, frame_idx_mod_59, u, v, frag_x, frag_y, r);
    float rgba[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int hit = -1;
    for (int i = 0; i < GV_MAX_STEPS; ++i) {
        float p[3];
        gv_step(r, p);
        sample(p, rgba);
        if (gv_hits(rgba[3])) { hit = i; break; }
    }
    if (hit_ro) for (int k = 0; k < 3; ++k) hit_ro[k] = r.ro[k];
    gv_resolve(hit >= 0, rgba, out);
    return hit;
}
