// k_post.hip -- K8 / K9 and K10 / K11: the post-process tail that consumes the shade pass.
//   K8  k_taa_resolve        shaders/taa_resolve.glsl:180-287   (full-screen draw, render.cpp:1131-1137)
//   K9  k_final_post_process shaders/final_post_process.glsl:2-10,31-34 (render.cpp:1181-1187)
//   K10 / K11 k_bloom_pass, k_bloom_small, k_bloom_down_pair, k_bloom_quad   shaders/bloom_downsample.glsl:38-98, bloom_upsample.glsl:23-58
//                            (render.cpp:1139-1176): the instantiations of one pass, chosen by pbrk_bloom_pass
//
// Sampler (SAMPLER_LINEAR_CLAMP on 2-D textures): texel coordinates are snapped to 1/256 texel before the bilinear
// split -- Vulkan's subTexelPrecisionBits = 8, what the reference's target GPUs do -- then weights and lerps are exact
// fp32 (a + t*(b-a), x then y); edges clamp.  A tap aimed at a texel centre therefore returns that texel bit for bit,
// which is what lets K8 read its 3x3 neighbourhood, its velocity tap and 5 of the 9 Catmull-Rom history taps as plain
// texel fetches (kCentreExact, valid while the snap absorbs the fp32 coordinate error: extents <= 8192).
// Arithmetic follows the shader statement by statement (no contraction, correctly rounded divide / sqrt), so K8 is
// bit-identical to the oracle and, through Oracle-A, to the shader text executed on the CPU.
// Both kernels are HBM-shaped by bytes (K8: 36 B per pixel = 8 lighting + 4 depth + 4 + 4 velocity + 8 history + 8
// written; K9: 8 B read + 4 B written); K8 issues 34 vector loads per pixel and is bound by the L1 path.
// Every step the kernels share is written once: the sampler's blend (bilerp, over a Tap from split_tap), the RGBA16F unpack
// (unpack_rgba16f; unpack_row for whole rows), the bloom shaders' weighted sums (down_fold / up_fold under down_sum / up_sum), the
// whole-row window loads of the exact 2 : 1 passes (bloom_row) and the one-pixel additive blend and store (blend_store).  What stays
// apart does so for a measured reason, given where it stands (profiles/post_one_copy.md has the numbers).
#include "pbr_device.h"
#include "pbr_kernels.h"

#include <hip/hip_fp16.h>

namespace {

__device__ __forceinline__ float h2f(unsigned short h) { return __half2float(__ushort_as_half(h)); }
// clamp to [0, hi], hi >= 0 and wave-uniform (a texture extent - 1): the median of (v, 0, hi) in one instruction -- the compare /
// select / min the plain expression compiles to is three, and the samplers below clamp two indices per axis and tap
__device__ __forceinline__ int clampi(int v, int /*lo == 0*/, int hi) {
    int r;
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(v), "s"(hi));
    return r;
}
__device__ __forceinline__ float lerpx(float p, float q, float t) { return p + t * (q - p); }
// The same value for a COMPILE-TIME fraction: when t is a power of two, t * (q - p) is exact (texels are fp16: no fp32 underflow within
// reach), so one FMA rounds exactly like the multiply-add pair; other fractions keep the sampler's two roundings.
__device__ __forceinline__ float lerpc(float p, float q, float t) { return (t == 0.5f || t == 0.25f) ? fmaf(t, q - p, p) : p + t * (q - p); }

struct Rgba { float x, y, z, w; };
__device__ __forceinline__ float2 lerpx(float2 p, float2 q, float t) { return make_float2(lerpx(p.x, q.x, t), lerpx(p.y, q.y, t)); }
__device__ __forceinline__ Rgba lerpx(const Rgba& p, const Rgba& q, float t) { return Rgba{lerpx(p.x, q.x, t), lerpx(p.y, q.y, t), lerpx(p.z, q.z, t), lerpx(p.w, q.w, t)}; }
// the sampler's blend of a tap's four texels (scalars or texels): x first, then y
template <class T>
__device__ __forceinline__ T bilerp(const T& t00, const T& t10, const T& t01, const T& t11, float a, float b) { return lerpx(lerpx(t00, t10, a), lerpx(t01, t11, a), b); }

__device__ __forceinline__ Rgba unpack_rgba16f(uint2 v) { return Rgba{h2f(v.x & 0xffff), h2f(v.x >> 16), h2f(v.y & 0xffff), h2f(v.y >> 16)}; }
__device__ __forceinline__ float2 unpack_rg16f(unsigned v) { return make_float2(h2f(v & 0xffff), h2f(v >> 16)); }
__device__ __forceinline__ void rgb_of(const Rgba& v, float* o) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
// N consecutive texels (rgb) from the 2 N words of a row (alpha is never converted: through unpack_rgba16f the pair kernels schedule differently)
template <int N>
__device__ __forceinline__ void unpack_row(const unsigned* w, float (*t)[3]) {
#pragma unroll
    for (int c = 0; c < N; ++c) { t[c][0] = h2f(w[2 * c] & 0xffff); t[c][1] = h2f(w[2 * c] >> 16); t[c][2] = h2f(w[2 * c + 1] & 0xffff); }
}

// pointer-addressed texel fetches
__device__ __forceinline__ Rgba texel_rgba16f(const PbrkTex2D& t, int i, int j) { return unpack_rgba16f(((const uint2*)t.data)[(size_t)j * t.width + i]); }
__device__ __forceinline__ float2 texel_rg16f(const PbrkTex2D& t, int i, int j) { return unpack_rg16f(((const unsigned*)t.data)[(size_t)j * t.width + i]); }
// buffer-addressed texel fetches: one 32-bit offset per load instead of a 64-bit address (textures are < 2 GiB, checked on the host)
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tex_rsrc(const PbrkTex2D& t, int texel_bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)t.data, 0, t.width * t.height * texel_bytes, 0x00020000);
}
__device__ __forceinline__ Rgba fetch_rgba16f(__amdgpu_buffer_rsrc_t rs, int w, int i, int j) {
    u32x2v v = __builtin_amdgcn_raw_buffer_load_b64(rs, (j * w + i) * 8, 0, 0);
    return unpack_rgba16f(make_uint2(v.x, v.y));
}
__device__ __forceinline__ float2 fetch_rg16f(__amdgpu_buffer_rsrc_t rs, int w, int i, int j) {
    return unpack_rg16f(__builtin_amdgcn_raw_buffer_load_b32(rs, (j * w + i) * 4, 0, 0));
}

// snapped bilinear split of one axis: returns the two clamped texel indices and the weight of the second
// (snap_split in k_shade_internal.h is the same arithmetic with another clamp instruction, for K5 / K16)
__device__ __forceinline__ void split_axis(float coord01, int extent, int& i0, int& i1, float& a) {
    float f = coord01 * (float)extent - 0.5f;
    f = floorf(f * 256.0f + 0.5f) * (1.0f / 256.0f);
    float fl = floorf(f);
    a = f - fl;
    int i = (int)fminf(fmaxf(fl, -1.0f), (float)extent);       // clamp before the conversion: no saturation / overflow for wild coordinates
    i0 = clampi(i, 0, extent - 1); i1 = clampi(i + 1, 0, extent - 1);
}
// one bilinear tap: the texel pairs of both axes and the weights of the second of each
struct Tap { int i0, i1, j0, j1; float a, b; };
__device__ __forceinline__ Tap split_tap(float u, float v, int width, int height) {
    Tap p;
    split_axis(u, width, p.i0, p.i1, p.a); split_axis(v, height, p.j0, p.j1, p.b);
    return p;
}
// the sampler: fetch four, bilerp; texel(i, j) is any of the fetches above
template <class Texel>
__device__ __forceinline__ auto sample(const Tap& p, Texel texel) { return bilerp(texel(p.i0, p.j0), texel(p.i1, p.j0), texel(p.i0, p.j1), texel(p.i1, p.j1), p.a, p.b); }

__device__ __forceinline__ Rgba sample_rgba16f(const PbrkTex2D& t, float u, float v) {
    return sample(split_tap(u, v, t.width, t.height), [&](int i, int j) { return texel_rgba16f(t, i, j); });
}
__device__ __forceinline__ float2 sample_rg16f(const PbrkTex2D& t, float u, float v) {
    return sample(split_tap(u, v, t.width, t.height), [&](int i, int j) { return texel_rg16f(t, i, j); });
}
__device__ __forceinline__ float sample_r32f(const PbrkTex2D& t, float u, float v) {
    return sample(split_tap(u, v, t.width, t.height), [&](int i, int j) { return ((const float*)t.data)[(size_t)j * t.width + i]; });
}

__device__ __forceinline__ float mitchell_netravali(float x) {            // taa_resolve.glsl:13-26
    const float B = 1.0f / 3.0f, C = 1.0f / 3.0f;
    float ax = fabsf(x);
    if (ax < 1.0f)
        return ((12.0f - 9.0f * B - 6.0f * C) * ax * ax * ax + (-18.0f + 12.0f * B + 6.0f * C) * ax * ax + (6.0f - 2.0f * B)) / 6.0f;
    else if (ax >= 1.0f && ax < 2.0f)
        return ((-B - 6.0f * C) * ax * ax * ax + (6.0f * B + 30.0f * C) * ax * ax + (-12.0f * B - 48.0f * C) * ax + (8.0f * B + 24.0f * C)) / 6.0f;
    return 0.0f;
}

__device__ __forceinline__ uint2 pack_half4(float r0, float r1, float r2) {
    uint2 v;
    v.x = (unsigned)__half_as_ushort(__float2half_rn(r0)) | ((unsigned)__half_as_ushort(__float2half_rn(r1)) << 16);
    v.y = (unsigned)__half_as_ushort(__float2half_rn(r2)) | (0x3c00u << 16);
    return v;
}

// kCentreExact (frames up to 8192^2 whose history has the frame's size): every tap the shader aims at a texel centre -- the 3x3 neighbourhood, depth, the
// velocity tap and the outer Catmull-Rom taps -- is one texel fetch, and the outer taps need neither their division by the
// texture size nor the bilinear split (their texel is floor(sp - 0.5) - 1 / + 2).  Otherwise every tap goes through the sampler.
struct TaaParams { PbrkTaaArgs a; float psx, psy; };       // 1 / width, 1 / height: the shader's divisions (:190), done once on the host
template <bool kCentreExact, bool kHalfOut>
__global__ __launch_bounds__(256) void k_taa_resolve(TaaParams P) {
    const PbrkTaaArgs& A = P.a;
    const int px = blockIdx.x * 64 + (threadIdx.x & 63);
    const int py = A.y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= A.width || py >= A.y1) return;
    const PbrkTex2D& LR = A.lighting_result;
    const PbrkTex2D& HI = A.prev_frame_result;
    const int W = LR.width, H = LR.height;
    const __amdgpu_buffer_rsrc_t rs_lr = tex_rsrc(LR, 8), rs_hi = tex_rsrc(HI, 8), rs_v = tex_rsrc(A.gbuffer_velocity, 4), rs_pv = tex_rsrc(A.gbuffer_velocity_prev, 4);
    const float tsx = (float)W, tsy = (float)H;                                 // :189
    const float psx = P.psx, psy = P.psy;                                       // :190 (1.0f / tsx, 1.0f / tsy: IEEE divisions, identical on the host)
    const float uvx = ((float)px + 0.5f) * psx, uvy = ((float)py + 0.5f) * psy; // :192

    float tot[3] = {0, 0, 0}, wsum = 0.0f, m1[3] = {0, 0, 0}, m2[3] = {0, 0, 0};
    float closest_depth = 10000.0f, cdu = 0.0f, cdv = 0.0f;
    float depth;                                                                // :221 (same tap nine times)
    if (kCentreExact) {
        // depth decides a branch (:222), so its tap keeps all of the sampler's arithmetic: the right and lower neighbours enter with a
        // zero weight, p + 0 * (q - p), which is p unless one of them is not finite; then it is NaN and no tap is the closest
        const float* D = (const float*)A.gbuffer_depth.data;
        const size_t r0 = (size_t)py * W, r1 = (size_t)min(py + 1, H - 1) * W;
        const int x1 = min(px + 1, W - 1);
        depth = bilerp(D[r0 + px], D[r0 + x1], D[r1 + px], D[r1 + x1], 0.0f, 0.0f);
    } else depth = sample_r32f(A.gbuffer_depth, uvx, uvy);
#pragma unroll
    for (int x = -1; x <= 1; ++x)                                               // :205-227
#pragma unroll
        for (int y = -1; y <= 1; ++y) {
            float su = uvx + (float)x * psx, sv = uvy + (float)y * psy;
            Rgba nb = kCentreExact ? fetch_rgba16f(rs_lr, W, clampi(px + x, 0, W - 1), clampi(py + y, 0, H - 1)) : sample_rgba16f(LR, su, sv);
            float w = mitchell_netravali(sqrtf((float)x * (float)x + (float)y * (float)y));
            float n[3] = {nb.x, nb.y, nb.z};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                tot[k] = tot[k] + n[k] * w;
                m1[k] = m1[k] + n[k];
                m2[k] = m2[k] + n[k] * n[k];
            }
            wsum = wsum + w;
            if (depth < closest_depth) { closest_depth = depth; cdu = su; cdv = sv; }   // :222-225: only the first tap (-1,-1) can win
        }
    const SharedRcp rws = shared_rcp(wsum);                                      // one reciprocal, three exact quotients (pbr_device.h)
    float src[3] = {div_by(tot[0], rws), div_by(tot[1], rws), div_by(tot[2], rws)};   // :228
    float2 vel;
    if (kCentreExact && closest_depth < 10000.0f) vel = fetch_rg16f(rs_v, W, clampi(px - 1, 0, W - 1), clampi(py - 1, 0, H - 1));
    else vel = sample_rg16f(A.gbuffer_velocity, cdu, cdv);                      // :230
    const float ru = uvx - vel.x * 0.5f, rv = uvy - vel.y * 0.5f;               // :231
    const float2 pvel = sample(split_tap(ru, rv, W, H), [&](int i, int j) { return fetch_rg16f(rs_pv, W, i, j); });   // :232

    // :234 history, 9 bilinear taps in the shader's order
    float prev[3] = {0, 0, 0};
    {
        const int HW = HI.width, HH = HI.height;
        float wxs[3], wys[3], ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0};
        int ci0[3], ci1[3], cj0[3], cj1[3];
        const float uvs[2] = {ru, rv}, tss[2] = {tsx, tsy};
#pragma unroll
        for (int axis = 0; axis < 2; ++axis) {                                  // :139-167
            int* i0 = axis ? cj0 : ci0; int* i1 = axis ? cj1 : ci1; float* wt = axis ? wys : wxs; float* frac = axis ? cb : ca;
            const int extent = axis ? HH : HW;
            float sp = uvs[axis] * tss[axis];
            float fl = floorf(sp - 0.5f);
            float tp1 = fl + 0.5f;
            float f = sp - tp1;
            wt[0] = f * (-0.5f + f * (1.0f - 0.5f * f));
            float w1 = 1.0f + f * f * (-2.5f + 1.5f * f);
            float w2 = f * (0.5f + f * (2.0f - 1.5f * f));
            wt[2] = f * f * (-0.5f + 0.5f * f);
            wt[1] = w1 + w2;
            float offset12 = w2 / (w1 + w2);
            split_axis((tp1 + offset12) / tss[axis], extent, i0[1], i1[1], frac[1]);
            if (kCentreExact) {
                int t = (int)fl;
                i0[0] = i1[0] = clampi(t - 1, 0, extent - 1); i0[2] = i1[2] = clampi(t + 2, 0, extent - 1);
            } else {
                split_axis((tp1 - 1.0f) / tss[axis], extent, i0[0], i1[0], frac[0]);
                split_axis((tp1 + 2.0f) / tss[axis], extent, i0[2], i1[2], frac[2]);
            }
        }
        auto texel = [&](int i, int j) { return fetch_rgba16f(rs_hi, HW, i, j); };
#pragma unroll
        for (int row = 0; row < 3; ++row)
#pragma unroll
            for (int col = 0; col < 3; ++col) {
                // bilerp's blends in bilerp's order, without those of a texel with itself (an exact axis has one texel for both of the tap's)
                const bool x_exact = kCentreExact && col != 1, y_exact = kCentreExact && row != 1;
                Rgba top = texel(ci0[col], cj0[row]);
                if (!x_exact) top = lerpx(top, texel(ci1[col], cj0[row]), ca[col]);
                Rgba s = top;
                if (!y_exact) {
                    Rgba bot = texel(ci0[col], cj1[row]);
                    if (!x_exact) bot = lerpx(bot, texel(ci1[col], cj1[row]), ca[col]);
                    s = lerpx(top, bot, cb[row]);
                }
                prev[0] = prev[0] + (s.x * wxs[col]) * wys[row];
                prev[1] = prev[1] + (s.y * wxs[col]) * wys[row];
                prev[2] = prev[2] + (s.z * wxs[col]) * wys[row];
            }
    }
    const float inv9 = 1.0f / 9.0f;                                             // :237
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                               // :239-244 (gamma = 1)
        float avg = m1[k] * inv9;
        float sigma = sqrtf(fabsf(m2[k] * inv9 - avg * avg));
        float minc = avg - sigma, maxc = avg + sigma;
        prev[k] = fminf(fmaxf(prev[k], minc), maxc);
    }
    float wB = 0.05f, wA = 1.0f - wB;                                           // :252-253
    float dvx = pvel.x - vel.x, dvy = pvel.y - vel.y;
    wB = wB + 1000.0f * sqrtf(dvx * dvx + dvy * dvy);                           // :269-270
    if (ru != fminf(fmaxf(ru, 0.0f), 1.0f) || rv != fminf(fmaxf(rv, 0.0f), 1.0f)) { wA = 0.0f; wB = 1.0f; }   // :272-275
    const float den = fmaxf(wB + wA, 0.00001f);
    // true divisions: `den` is data (a shared-reciprocal quotient would be 1 ulp off whenever its significand is all ones:
    // a handful of pixels per 1080p frame, and this kernel is bit-exact)
    float r0 = (src[0] * wB + prev[0] * wA) / den, r1 = (src[1] * wB + prev[1] * wA) / den, r2 = (src[2] * wB + prev[2] * wA) / den;   // :277
    const size_t o = (size_t)py * A.width + px;
    if (kHalfOut) ((uint2*)A.out)[o] = pack_half4(r0, r1, r2);
    else ((float4*)A.out)[o] = make_float4(r0, r1, r2, 1.0f);                   // :290
}

__device__ __forceinline__ float aces_approx(float v) {                   // final_post_process.glsl:2-10
    v = v * 0.6f;
    const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
    return fminf(fmaxf((v * (a * v + b)) / (v * (c * v + d) + e), 0.0f), 1.0f);
}
__device__ __forceinline__ unsigned to_unorm8(float v) {                   // render-target conversion, round to nearest even
    return (unsigned)__float2int_rn(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);
}

// pow(x, 1/2.2) for x in [0,1] through the hardware log2 / exp2 (1 ulp each): relative error < 1e-6, far inside the
// 8-bit target's step and the 1e-5 the float targets are checked to; libm's powf costs ~10x more instructions.
__device__ __forceinline__ float pow_gamma(float x) {
    return __builtin_amdgcn_exp2f((1.0f / 2.2f) * __builtin_amdgcn_logf(x));
}
__device__ __forceinline__ void tone_map(const Rgba& s, float& r0, float& r1, float& r2) {     // :32-33
    r0 = pow_gamma(aces_approx(2.0f * s.x)); r1 = pow_gamma(aces_approx(2.0f * s.y)); r2 = pow_gamma(aces_approx(2.0f * s.z));
}
template <int kOutFmt> __device__ __forceinline__ unsigned pack8(float r0, float r1, float r2) {
    return kOutFmt == PBRK_FMT_RGBA8UN ? (to_unorm8(r0) | (to_unorm8(r1) << 8) | (to_unorm8(r2) << 16) | 0xff000000u)
                                       : (to_unorm8(r2) | (to_unorm8(r1) << 8) | (to_unorm8(r0) << 16) | 0xff000000u);
}

// general form: any source size (bilinear), one pixel per thread
template <int kOutFmt>
__global__ __launch_bounds__(256) void k_final_post_process(PbrkFinalArgs A) {
    const int px = blockIdx.x * 64 + (threadIdx.x & 63);
    const int py = A.y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= A.width || py >= A.y1) return;
    Rgba s = sample_rgba16f(A.src, ((float)px + 0.5f) / (float)A.width, ((float)py + 0.5f) / (float)A.height);
    float r0, r1, r2;
    tone_map(s, r0, r1, r2);
    const size_t o = (size_t)py * A.width + px;
    if (kOutFmt == PBRK_FMT_RGBA8UN || kOutFmt == PBRK_FMT_BGRA8UN) ((unsigned*)A.out)[o] = pack8<kOutFmt>(r0, r1, r2);
    else if (kOutFmt == PBRK_FMT_RGBA16F) ((uint2*)A.out)[o] = pack_half4(r0, r1, r2);
    else ((float4*)A.out)[o] = make_float4(r0, r1, r2, 1.0f);
}

// the reference's case: source and target have one size, every tap is a texel centre -> a streaming map, 4 pixels
// (32 B in, 16 B out for the 8-bit targets) per thread; width % 4 == 0
template <int kOutFmt>
__global__ __launch_bounds__(256) void k_final_post_process_stream(PbrkFinalArgs A) {
    const int quads_per_row = A.width >> 2;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nq = (size_t)quads_per_row * (A.y1 - A.y0);
    if (q >= nq) return;
    const size_t first = (size_t)A.y0 * A.width + q * 4;                        // rows are contiguous: a flat range of pixels
    const uint4* src = (const uint4*)((const uint2*)A.src.data + first);
    uint4 v0 = src[0], v1 = src[1];
    const unsigned raw[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    float t[4][3], r[4][3];
    unpack_row<4>(raw, t);
#pragma unroll
    for (int k = 0; k < 4; ++k) tone_map(Rgba{t[k][0], t[k][1], t[k][2], 1.0f}, r[k][0], r[k][1], r[k][2]);
    if (kOutFmt == PBRK_FMT_RGBA8UN || kOutFmt == PBRK_FMT_BGRA8UN) {
        ((uint4*)((unsigned*)A.out + first))[0] = make_uint4(pack8<kOutFmt>(r[0][0], r[0][1], r[0][2]), pack8<kOutFmt>(r[1][0], r[1][1], r[1][2]),
                                                             pack8<kOutFmt>(r[2][0], r[2][1], r[2][2]), pack8<kOutFmt>(r[3][0], r[3][1], r[3][2]));
    } else if (kOutFmt == PBRK_FMT_RGBA16F) {
        uint2 a = pack_half4(r[0][0], r[0][1], r[0][2]), b = pack_half4(r[1][0], r[1][1], r[1][2]);
        uint2 c = pack_half4(r[2][0], r[2][1], r[2][2]), d = pack_half4(r[3][0], r[3][1], r[3][2]);
        uint4* o = (uint4*)((uint2*)A.out + first);
        o[0] = make_uint4(a.x, a.y, b.x, b.y); o[1] = make_uint4(c.x, c.y, d.x, d.y);
    } else {
        float4* o = (float4*)A.out + first;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = make_float4(r[k][0], r[k][1], r[k][2], 1.0f);
    }
}

// K10 / K11: bloom passes
struct BloomParams { PbrkBloomArgs a; float x_step, y_step, rcp_dw, rcp_dh; int exact2to1; };

// The shaders' sums, bloom_downsample.glsl:50-97 and bloom_upsample.glsl:43-58: four-tap groups added left to right, then folded with the
// weights in the shaders' order; the firefly clamp of the first downsample and the upsample's factor / 16 as the shaders write them.
__device__ __forceinline__ float group4(float a, float b, float c, float d) { return ((a + b) + c) + d; }
__device__ __forceinline__ float down_fold(float centre, float corners, float edges, float inner, int dst_mip_level) {
    float sum = centre * 0.125f;
    sum = sum + corners * 0.03125f;
    sum = sum + edges * 0.0625f;
    sum = sum + inner * 0.125f;
    if (dst_mip_level == 1) sum = fminf(sum, 1.0f);
    return sum;
}
__device__ __forceinline__ float up_fold(float centre, float edges, float corners, int dst_mip_level) {
    const float factor = dst_mip_level == 0 ? 0.06f : 1.0f;
    float sum = centre * 4.0f;
    sum = sum + edges * 2.0f;
    sum = sum + corners;
    return sum * factor / 16.0f;
}
// the same over tap(kx, ky), one channel of the tap at offset (kx - 2, ky - 2) texels (down) or (kx - 1, ky - 1) radii (up)
template <class TapFn>
__device__ __forceinline__ float down_sum(TapFn tap, int dst_mip_level) {
    return down_fold(tap(2, 2), group4(tap(0, 0), tap(4, 0), tap(0, 4), tap(4, 4)), group4(tap(2, 0), tap(0, 2), tap(4, 2), tap(2, 4)),
                     group4(tap(1, 1), tap(3, 1), tap(1, 3), tap(3, 3)), dst_mip_level);
}
template <class TapFn>
__device__ __forceinline__ float up_sum(TapFn tap, int dst_mip_level) {
    return up_fold(tap(1, 1), group4(tap(1, 0), tap(0, 1), tap(2, 1), tap(1, 2)), group4(tap(0, 0), tap(2, 0), tap(0, 2), tap(2, 2)), dst_mip_level);
}

// the tail of a one-pixel pass: the additive blend with the operand (blend_src, or the target itself) and the store
__device__ __forceinline__ void blend_store(const PbrkBloomArgs& A, int px, int py, float* r) {
    uint2* o = (uint2*)A.dst + (size_t)py * A.dst_width + px;
    if (A.blend_additive) {
        const Rgba d = unpack_rgba16f(A.blend_src ? ((const uint2*)A.blend_src)[(size_t)py * A.dst_width + px] : *o);
        r[0] = r[0] + d.x; r[1] = r[1] + d.y; r[2] = r[2] + d.z;
    }
    *o = pack_half4(r[0], r[1], r[2]);
}
// The general path of a bloom pass: every tap through the snapped bilinear sampler (any size ratio, border pixels of the exact passes).
// Column / row tap coordinates repeat (5 distinct offsets for the 13-tap downsample, 3 for the tent), so the snapped bilinear split is
// done once per distinct offset and the taps index the results.
template <bool kUp>
__device__ __forceinline__ void bloom_general(const BloomParams& P, const __amdgpu_buffer_rsrc_t rs, const int px, const int py, float* r) {
    const PbrkBloomArgs& A = P.a;
    const int SW = A.src.width, SH = A.src.height;
    SharedRcp rw, rh;
    rw.d = (float)A.dst_width; rw.r = P.rcp_dw; rh.d = (float)A.dst_height; rh.r = P.rcp_dh;
    const float u = div_by((float)px + 0.5f, rw), v = div_by((float)py + 0.5f, rh);       // fs_uv (full-screen triangle)
    constexpr int kOffs = kUp ? 3 : 5;                                                  // offsets -1..1 (x radius) or -2..2 (x texel)
    int ci0[kOffs], ci1[kOffs], cj0[kOffs], cj1[kOffs]; float ca[kOffs], cb[kOffs];
#pragma unroll
    for (int k = 0; k < kOffs; ++k) {
        const float off = (float)(k - kOffs / 2);
        split_axis(u + off * P.x_step, SW, ci0[k], ci1[k], ca[k]);
        split_axis(v + off * P.y_step, SH, cj0[k], cj1[k], cb[k]);
    }
    auto texel = [&](int i, int j) { return fetch_rgba16f(rs, SW, i, j); };
    float t[kOffs][kOffs][3];                                                           // [ky][kx]: all nine (up); the 13 whose offsets are both even or both odd (down)
    auto fill = [&](int kx, int ky) { rgb_of(sample(Tap{ci0[kx], ci1[kx], cj0[ky], cj1[ky], ca[kx], cb[ky]}, texel), t[ky][kx]); };
    constexpr int kStep = kUp ? 1 : 2;                                                  // the shaders' order, a..i then j k l m: row by row costs k_bloom_pass<false> a wave
#pragma unroll
    for (int k = 0; k < 9; ++k) fill(kStep * (k % 3), kStep * (k / 3));
    if (!kUp) { fill(1, 1); fill(3, 1); fill(1, 3); fill(3, 3); }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        auto tap = [&](int kx, int ky) { return t[ky][kx][c]; };
        if constexpr (kUp) r[c] = up_sum(tap, A.dst_mip_level);
        else r[c] = down_sum(tap, A.dst_mip_level);
    }
}

// N consecutive texels (rgb) of row y starting at column x0: whole-row loads when the run lies inside the level, else texel by texel
// with the sampler's clamp to edge (a tap whose two texels clamp to the same one returns it whatever its fraction: p + t (p - p)).
template <int N>
__device__ __forceinline__ void bloom_row(const __amdgpu_buffer_rsrc_t rs, const int SW, const int SH, const int x0, const int y, const bool inside, float (*t)[3]) {
    static_assert(N == 5 || N == 6 || N == 8, "window width");
    if (inside) {
        const int off = (y * SW + x0) * 8;
        unsigned w[16];                                                                 // loads written out, two first: as a loop k_bloom_down_pair schedules 5 % slower
        const u32x4v q0 = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0), q1 = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16, 0, 0);
        w[0] = q0.x; w[1] = q0.y; w[2] = q0.z; w[3] = q0.w; w[4] = q1.x; w[5] = q1.y; w[6] = q1.z; w[7] = q1.w;
        if (N == 5) { const u32x2v q2 = __builtin_amdgcn_raw_buffer_load_b64(rs, off + 32, 0, 0); w[8] = q2.x; w[9] = q2.y; }
        else { const u32x4v q2 = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 32, 0, 0); w[8] = q2.x; w[9] = q2.y; w[10] = q2.z; w[11] = q2.w; }
        if (N == 8) { const u32x4v q3 = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 48, 0, 0); w[12] = q3.x; w[13] = q3.y; w[14] = q3.z; w[15] = q3.w; }
        unpack_row<N>(w, t);
    } else {
        const int yc = clampi(y, 0, SH - 1);
#pragma unroll
        for (int c = 0; c < N; ++c) rgb_of(fetch_rgba16f(rs, SW, clampi(x0 + c, 0, SW - 1), yc), t[c]);
    }
}

template <bool kUp>
__global__ __launch_bounds__(256) void k_bloom_pass(BloomParams P) {
    const PbrkBloomArgs& A = P.a;
    const int px = blockIdx.x * 64 + (threadIdx.x & 63);
    const int py = A.y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= A.dst_width || py >= A.y1) return;
    const int SW = A.src.width, SH = A.src.height;
    const __amdgpu_buffer_rsrc_t rs = tex_rsrc(A.src, 8);
    float r[3];
    bool done = false;
    // Exact 2:1 passes (every level of an even-sized chain; the two full-size passes of a 1080p frame): the snapped tap
    // coordinates are known in closed form -- texel pairs at fraction 1/2 (down) or 1/4, 3/4 by pixel parity (up) -- so an
    // interior pixel reads its 6x6 / 5x5 source window as whole rows (18 / 15 loads instead of 52 / 36) and needs no
    // coordinate arithmetic.  Same lerps in the same order: bit-identical to the general path below (border pixels take it).
    if (P.exact2to1) {
        if (!kUp) {
            if (px >= 1 && px <= A.dst_width - 2 && py >= 1 && py <= A.dst_height - 2) {
                float hx[6][5][3];                                                      // rows x horizontal taps (offsets -2..2) x rgb
#pragma unroll
                for (int rr = 0; rr < 6; ++rr) {
                    float t[6][3];
                    bloom_row<6>(rs, SW, SH, 2 * px - 2, 2 * py - 2 + rr, true, t);
#pragma unroll
                    for (int k = 0; k < 5; ++k)
#pragma unroll
                        for (int c = 0; c < 3; ++c) hx[rr][k][c] = lerpc(t[k][c], t[k + 1][c], 0.5f);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) r[c] = down_sum([&](int kx, int ky) { return lerpc(hx[ky][kx][c], hx[ky + 1][kx][c], 0.5f); }, A.dst_mip_level);
                done = true;
            }
        } else {
            const int i = px >> 1, j = py >> 1;
            if (i >= 2 && i <= SW - 3 && j >= 2 && j <= SH - 3) {
                // lerpx, not lerpc: these fractions differ by lane, and lerpc would pay for both of its forms and a select (107 VGPRs for 86)
                const bool ox = px & 1, oy = py & 1;
                const float fx_side = ox ? 0.75f : 0.25f, fx_mid = ox ? 0.25f : 0.75f;      // fractions of the taps at -1.5 / +1.5 and at 0
                const float fy_side = oy ? 0.75f : 0.25f, fy_mid = oy ? 0.25f : 0.75f;
                float hx[5][3][3];                                                      // rows x horizontal taps (left, centre, right) x rgb
#pragma unroll
                for (int rr = 0; rr < 5; ++rr) {
                    float t[5][3];
                    bloom_row<5>(rs, SW, SH, i - 2, j - 2 + rr, true, t);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        hx[rr][0][c] = lerpx(t[0][c], t[1][c], fx_side);
                        hx[rr][1][c] = lerpx(ox ? t[2][c] : t[1][c], ox ? t[3][c] : t[2][c], fx_mid);
                        hx[rr][2][c] = lerpx(t[3][c], t[4][c], fx_side);
                    }
                }
                auto tapu = [&](int kx, int ky, int c) {
                    if (ky == 0) return lerpx(hx[0][kx][c], hx[1][kx][c], fy_side);
                    if (ky == 2) return lerpx(hx[3][kx][c], hx[4][kx][c], fy_side);
                    return lerpx(oy ? hx[2][kx][c] : hx[1][kx][c], oy ? hx[3][kx][c] : hx[2][kx][c], fy_mid);
                };
#pragma unroll
                for (int c = 0; c < 3; ++c) r[c] = up_sum([&](int kx, int ky) { return tapu(kx, ky, c); }, A.dst_mip_level);
                done = true;
            }
        }
    }
    if (!done) bloom_general<kUp>(P, rs, px, py, r);
    blend_store(A, px, py, r);
}

// K10 / K11, SMALL levels through the general sampler (the passes of a 1080p frame below 240 x 135, whose sizes are not 2 : 1): a level
// of a few thousand pixels cannot fill the chip, so a pass lasts as long as ONE thread's chain of 52 / 36 dependent-address fetches
// and ~1000 instructions.  Here four lanes share a pixel, one per group of the shader's sum (downsample: centre | four corners at
// +-2 | four edges at +-2 | four inner taps at +-1; upsample: centre | four edges | four corners | idle): a lane runs at most four
// taps, sums them in the shader's order, and lane 0 of the pixel folds the group sums -- again in the shader's order -- after three
// shuffles per channel.  Same taps, same operations, same order: bit-identical; the chain is a third as long.
template <bool kUp>
__global__ __launch_bounds__(256) void k_bloom_small(BloomParams P) {
    const PbrkBloomArgs& A = P.a;
    const int q = threadIdx.x & 3;
    const int px = blockIdx.x * 64 + (threadIdx.x >> 2);
    const int py = A.y0 + blockIdx.y;
    const bool live = px < A.dst_width;                                                 // whole quads of lanes: the shuffles below stay inside a pixel
    const int pxc = min(px, A.dst_width - 1);
    const int SW = A.src.width, SH = A.src.height;
    const __amdgpu_buffer_rsrc_t rs = tex_rsrc(A.src, 8);
    SharedRcp rw, rh;
    rw.d = (float)A.dst_width; rw.r = P.rcp_dw; rh.d = (float)A.dst_height; rh.r = P.rcp_dh;
    const float u = div_by((float)pxc + 0.5f, rw), v = div_by((float)py + 0.5f, rh);      // fs_uv, as in bloom_general
    const bool centre = q == 0 || (kUp && q == 3);
    const bool edge = kUp ? q == 1 : q == 2;
    const float mag = centre ? 0.0f : (kUp || q == 3) ? 1.0f : 2.0f;                     // tap offsets in units of x_step / y_step
    float g[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // corners (and the inner taps): (-,-) (+,-) (-,+) (+,+);  edges: (0,-) (-,0) (+,0) (0,+);  centre: (0,0)
        const float cx = (j & 1) ? 1.0f : -1.0f, cy = (j & 2) ? 1.0f : -1.0f;
        const float ex = j == 1 ? -1.0f : j == 2 ? 1.0f : 0.0f, ey = j == 0 ? -1.0f : j == 3 ? 1.0f : 0.0f;
        const float offx = (edge ? ex : cx) * mag, offy = (edge ? ey : cy) * mag;        // exact: +-2, +-1 or 0 (a centre lane repeats its tap)
        float t[3];
        rgb_of(sample(split_tap(u + offx * P.x_step, v + offy * P.y_step, SW, SH), [&](int x, int y) { return fetch_rgba16f(rs, SW, x, y); }), t);
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = j == 0 ? t[c] : (centre ? g[c] : g[c] + t[c]);   // ((t0 + t1) + t2) + t3; the centre group is its one tap
    }
    const int base = (threadIdx.x & 63) & ~3;
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float g1 = __shfl(g[c], base + 1), g2 = __shfl(g[c], base + 2), g3 = __shfl(g[c], base + 3);
        r[c] = kUp ? up_fold(g[c], g1, g2, A.dst_mip_level) : down_fold(g[c], g1, g2, g3, A.dst_mip_level);
    }
    if (live && q == 0) blend_store(A, px, py, r);
}

// K11, exact 1 : 2 upsample of LARGE levels: one thread per 2 x 2 block of target pixels.  The four pixels (2i + ox, 2j + oy) read the SAME
// 5 x 5 source window around texel (i, j); only their tap fractions differ (1/4 or 3/4 by parity): 15 loads and 75 conversions per four
// pixels instead of per pixel.  Every tap is the same lerp of the same texels with the same fraction as in k_bloom_pass, and every pixel's sum
// runs in the shader's order: bit-identical (tests/test_post.py compares all twelve targets with the shader text at 1920 x 1080).
// Blocks at the border of the level read their window texel by texel with the sampler's edge clamp (the closed-form fractions hold for
// every pixel; only the whole-row loads need the window inside the level).  Small levels stay with one pixel per thread: they are
// latency-bound and a four-pixel thread is four times as long.  (The downsample had a 2 x 2 form too -- 8 x 8 window, 25 distinct taps for
// 52 -- which kept 158 registers and two waves per SIMD on the 960 x 540 pass, 65 % of their lifetime waiting for 32 loads: the pair form
// below replaced it, 16.8 -> 14.2 us.)
// The window code and the pair tail are this kernel's own: one function for the window shared with k_bloom_pass<true>, or a blend-and-store
// shared with a one-pair-per-thread downsample, each made the 960 x 540 pass slower (7.9 -> 8.3 / 8.0 us).
__global__ __launch_bounds__(256) void k_bloom_quad(BloomParams P) {
    const PbrkBloomArgs& A = P.a;
    const int qx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int qy = (A.y0 >> 1) + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (2 * qx >= A.dst_width || 2 * qy >= A.y1) return;
    const int SW = A.src.width, SH = A.src.height;
    const __amdgpu_buffer_rsrc_t rs = tex_rsrc(A.src, 8);
    float r[2][2][3];                                                                   // [oy][ox][rgb]
    const bool interior = qx >= 2 && qx <= SW - 3 && qy >= 2 && qy <= SH - 3;
    {
        // horizontal taps of a row: [parity][left, centre, right]
        float hx[5][2][3][3];
#pragma unroll
        for (int rr = 0; rr < 5; ++rr) {
            float t[5][3];
            bloom_row<5>(rs, SW, SH, qx - 2, qy - 2 + rr, interior, t);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                hx[rr][0][0][c] = lerpc(t[0][c], t[1][c], 0.25f); hx[rr][1][0][c] = lerpc(t[0][c], t[1][c], 0.75f);
                hx[rr][0][1][c] = lerpc(t[1][c], t[2][c], 0.75f); hx[rr][1][1][c] = lerpc(t[2][c], t[3][c], 0.25f);
                hx[rr][0][2][c] = lerpc(t[3][c], t[4][c], 0.25f); hx[rr][1][2][c] = lerpc(t[3][c], t[4][c], 0.75f);
            }
        }
#pragma unroll
        for (int oy = 0; oy < 2; ++oy)
#pragma unroll
            for (int ox = 0; ox < 2; ++ox) {
                const float fy_side = oy ? 0.75f : 0.25f, fy_mid = oy ? 0.25f : 0.75f;
                auto tapu = [&](int kx, int ky, int c) {
                    if (ky == 0) return lerpc(hx[0][ox][kx][c], hx[1][ox][kx][c], fy_side);
                    if (ky == 2) return lerpc(hx[3][ox][kx][c], hx[4][ox][kx][c], fy_side);
                    return lerpc(hx[oy ? 2 : 1][ox][kx][c], hx[oy ? 3 : 2][ox][kx][c], fy_mid);
                };
#pragma unroll
                for (int c = 0; c < 3; ++c) r[oy][ox][c] = up_sum([&](int kx, int ky) { return tapu(kx, ky, c); }, A.dst_mip_level);
            }
    }
#pragma unroll
    for (int oy = 0; oy < 2; ++oy) {
        uint4* o = (uint4*)((uint2*)A.dst + (size_t)(2 * qy + oy) * A.dst_width + 2 * qx);
        if (A.blend_additive) {
            const uint4 d = A.blend_src ? *(const uint4*)((const uint2*)A.blend_src + (size_t)(2 * qy + oy) * A.dst_width + 2 * qx) : *o;
            const Rgba d0 = unpack_rgba16f(make_uint2(d.x, d.y)), d1 = unpack_rgba16f(make_uint2(d.z, d.w));
            r[oy][0][0] = r[oy][0][0] + d0.x; r[oy][0][1] = r[oy][0][1] + d0.y; r[oy][0][2] = r[oy][0][2] + d0.z;
            r[oy][1][0] = r[oy][1][0] + d1.x; r[oy][1][1] = r[oy][1][1] + d1.y; r[oy][1][2] = r[oy][1][2] + d1.z;
        }
        const uint2 a = pack_half4(r[oy][0][0], r[oy][0][1], r[oy][0][2]), b = pack_half4(r[oy][1][0], r[oy][1][1], r[oy][1][2]);
        *o = make_uint4(a.x, a.y, b.x, b.y);
    }
}

// K10, exact 2 : 1 downsample of LARGE levels: two horizontally adjacent target pixels per thread.  They share an 8 x 6 source window (24
// loads instead of 36) and 8 of their 2 x 13 taps coincide (a pixel's tap two texels to the right is its neighbour's centre tap): 18 distinct
// taps.  E[b][a]: tap at window position (2a, 2b); O[b][a]: tap at (2a + 1, 2b + 1); rows stream through (a tap needs two adjacent rows).
// Same lerps, same order of every pixel's sum as k_bloom_pass: bit-identical.
__global__ __launch_bounds__(256) void k_bloom_down_pair(BloomParams P) {
    const PbrkBloomArgs& A = P.a;
    const int qx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int py = A.y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (2 * qx >= A.dst_width || py >= A.y1) return;
    const int SW = A.src.width, SH = A.src.height;
    const __amdgpu_buffer_rsrc_t rs = tex_rsrc(A.src, 8);
    const bool interior = qx >= 1 && 2 * qx + 1 <= A.dst_width - 2 && py >= 1 && py <= A.dst_height - 2;
    float E[3][4][3], O[2][3][3], prev[7][3];
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
        float t[8][3], cur[7][3];
        bloom_row<8>(rs, SW, SH, 4 * qx - 2, 2 * py - 2 + rr, interior, t);
#pragma unroll
        for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) cur[k][c] = lerpc(t[k][c], t[k + 1][c], 0.5f);
        if (rr >= 1) {
            const int wy = rr - 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if ((wy & 1) == 0) {
#pragma unroll
                    for (int a = 0; a < 4; ++a) E[wy >> 1][a][c] = lerpc(prev[2 * a][c], cur[2 * a][c], 0.5f);
                } else {
#pragma unroll
                    for (int a = 0; a < 3; ++a) O[wy >> 1][a][c] = lerpc(prev[2 * a + 1][c], cur[2 * a + 1][c], 0.5f);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) prev[k][c] = cur[k][c];
    }
    float r[2][3];
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            r[dx][c] = down_sum([&](int kx, int ky) { return (kx & 1) ? O[ky >> 1][dx + (kx >> 1)][c] : E[ky >> 1][dx + (kx >> 1)][c]; }, A.dst_mip_level);
    const uint2 a = pack_half4(r[0][0], r[0][1], r[0][2]), b = pack_half4(r[1][0], r[1][1], r[1][2]);
    *(uint4*)((uint2*)A.dst + (size_t)py * A.dst_width + 2 * qx) = make_uint4(a.x, a.y, b.x, b.y);
}

__global__ void k_debug_sample_post(PbrkTex2D t, const float* __restrict__ coords, int count, float4* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    Rgba r = sample_rgba16f(t, coords[i * 3], coords[i * 3 + 1]);
    out[i] = make_float4(r.x, r.y, r.z, r.w);
}

bool tex_ok(const PbrkTex2D& t, int fmt) { return t.data && t.format == fmt && t.width > 0 && t.height > 0; }
bool band_ok(int y0, int y1, int height) { return y0 >= 0 && y0 < y1 && y1 <= height; }
int launched() { return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH; }
}  // namespace

extern "C" int pbrk_taa_resolve(const PbrkTaaArgs* a, void* stream) {
    if (!a || !a->out || a->width < 1 || a->height < 1 || !band_ok(a->y0, a->y1, a->height)) return PBRK_E_ARG;
    if (!tex_ok(a->lighting_result, PBRK_FMT_RGBA16F) || !tex_ok(a->prev_frame_result, PBRK_FMT_RGBA16F) || !tex_ok(a->gbuffer_depth, PBRK_FMT_R32F) ||
        !tex_ok(a->gbuffer_velocity, PBRK_FMT_RG16F) || !tex_ok(a->gbuffer_velocity_prev, PBRK_FMT_RG16F)) return PBRK_E_FORMAT;
    if (a->out_format != PBRK_FMT_RGBA16F && a->out_format != PBRK_FMT_RGBA32F) return PBRK_E_FORMAT;
    // the frame, its G-buffer planes and the render target share one size in the reference (render.cpp:680-697, 732-739)
    const PbrkTex2D* same[4] = {&a->lighting_result, &a->gbuffer_depth, &a->gbuffer_velocity, &a->gbuffer_velocity_prev};
    for (int k = 0; k < 4; ++k) if (same[k]->width != a->width || same[k]->height != a->height) return PBRK_E_ARG;
    if (a->out == a->prev_frame_result.data || a->out == a->lighting_result.data) return PBRK_E_ARG;
    if ((long long)a->width * a->height > (1ll << 27) || (long long)a->prev_frame_result.width * a->prev_frame_result.height > (1ll << 27)) return PBRK_E_ARG;   // 32-bit byte offsets
    // the exact path counts its outer history taps in texels of the frame: only a history of the frame's size has them at its own centres
    const bool centre = a->width <= 8192 && a->height <= 8192 && a->prev_frame_result.width == a->width && a->prev_frame_result.height == a->height;
    const bool half = a->out_format == PBRK_FMT_RGBA16F;
    static void (*const kernels[2][2])(TaaParams) = {{k_taa_resolve<false, false>, k_taa_resolve<false, true>}, {k_taa_resolve<true, false>, k_taa_resolve<true, true>}};
    TaaParams tp; tp.a = *a; tp.psx = 1.0f / (float)a->lighting_result.width; tp.psy = 1.0f / (float)a->lighting_result.height;
    hipLaunchKernelGGL(kernels[centre][half], dim3((a->width + 63) / 64, (a->y1 - a->y0 + 3) / 4), dim3(256), 0, (hipStream_t)stream, tp);
    return launched();
}

extern "C" int pbrk_final_post_process(const PbrkFinalArgs* a, void* stream) {
    if (!a || !a->out || a->width < 1 || a->height < 1 || !band_ok(a->y0, a->y1, a->height)) return PBRK_E_ARG;
    if (!tex_ok(a->src, PBRK_FMT_RGBA16F)) return PBRK_E_FORMAT;
    if (a->out == a->src.data) return PBRK_E_ARG;
    static const struct { int format; void (*general)(PbrkFinalArgs); void (*stream)(PbrkFinalArgs); } kernels[] = {
        {PBRK_FMT_RGBA8UN, k_final_post_process<PBRK_FMT_RGBA8UN>, k_final_post_process_stream<PBRK_FMT_RGBA8UN>},
        {PBRK_FMT_BGRA8UN, k_final_post_process<PBRK_FMT_BGRA8UN>, k_final_post_process_stream<PBRK_FMT_BGRA8UN>},
        {PBRK_FMT_RGBA16F, k_final_post_process<PBRK_FMT_RGBA16F>, k_final_post_process_stream<PBRK_FMT_RGBA16F>},
        {PBRK_FMT_RGBA32F, k_final_post_process<PBRK_FMT_RGBA32F>, k_final_post_process_stream<PBRK_FMT_RGBA32F>}};
    const bool stream_map = a->src.width == a->width && a->src.height == a->height && a->width <= 8192 && a->height <= 8192 && (a->width & 3) == 0;
    const dim3 grid = stream_map ? dim3((unsigned)((((size_t)(a->width >> 2) * (a->y1 - a->y0)) + 255) / 256)) : dim3((a->width + 63) / 64, (a->y1 - a->y0 + 3) / 4);
    for (const auto& k : kernels)
        if (k.format == a->out_format) {
            hipLaunchKernelGGL(stream_map ? k.stream : k.general, grid, dim3(256), 0, (hipStream_t)stream, *a);
            return launched();
        }
    return PBRK_E_FORMAT;
}

// which instantiation a bloom pass takes (all bit-identical): < 0 = the environment variable or the default
static long long g_quad_min = -1, g_small_max = -1;
extern "C" void pbrk_bloom_set_thresholds(long long quad_min_pixels, long long small_max_pixels) { g_quad_min = quad_min_pixels; g_small_max = small_max_pixels; }
static long long threshold(long long& value, const char* env, long long fallback) {
    if (value < 0) { const char* e = getenv(env); value = e ? atoll(e) : fallback; }
    return value;
}

extern "C" int pbrk_bloom_pass(const PbrkBloomArgs* a, void* stream) {
    if (!a || !a->dst || a->dst_width < 1 || a->dst_height < 1 || !band_ok(a->y0, a->y1, a->dst_height)) return PBRK_E_ARG;
    if (!tex_ok(a->src, PBRK_FMT_RGBA16F)) return PBRK_E_FORMAT;
    if ((long long)a->src.width * a->src.height > (1ll << 27) || a->dst == a->src.data) return PBRK_E_ARG;
    BloomParams p;
    p.a = *a;
    p.x_step = (a->upsample ? 1.5f : 1.0f) / (float)a->src.width;                       // radius / size, 1 / size (the shaders' x, y)
    p.y_step = (a->upsample ? 1.5f : 1.0f) / (float)a->src.height;
    p.rcp_dw = 1.0f / (float)a->dst_width; p.rcp_dh = 1.0f / (float)a->dst_height;
    // closed-form taps need the exact ratio and the snap to absorb the fp32 coordinate error (extents <= 8192), see the kernel
    const bool small = a->src.width <= 8192 && a->src.height <= 8192 && a->dst_width <= 8192 && a->dst_height <= 8192;
    p.exact2to1 = small && (a->upsample ? (a->dst_width == 2 * a->src.width && a->dst_height == 2 * a->src.height)
                                        : (a->src.width == 2 * a->dst_width && a->src.height == 2 * a->dst_height));
    const int rows = a->y1 - a->y0;
    const long long pixels = (long long)a->dst_width * rows;
    // two (downsample) / 2 x 2 (upsample) pixels per thread where the level is large enough to fill the chip with such threads (PBR_BLOOM_QUAD_MIN_PIXELS)
    const bool wide = p.exact2to1 && ((uintptr_t)a->dst & 15) == 0 && ((uintptr_t)a->src.data & 15) == 0 && ((uintptr_t)a->blend_src & 15) == 0 &&
                      pixels >= threshold(g_quad_min, "PBR_BLOOM_QUAD_MIN_PIXELS", 100000);
    void (*kernel)(BloomParams);
    dim3 grid((a->dst_width + 63) / 64, (rows + 3) / 4);                                // one pixel per thread
    if (wide && !a->upsample && !a->blend_additive && !(a->dst_width & 1)) {
        kernel = k_bloom_down_pair; grid.x = (a->dst_width / 2 + 63) / 64;
    } else if (wide && a->upsample && !((a->dst_width | a->dst_height | a->y0 | a->y1) & 1)) {
        kernel = k_bloom_quad; grid = dim3((a->dst_width / 2 + 63) / 64, (rows / 2 + 3) / 4);
    } else if (!p.exact2to1 && pixels <= threshold(g_small_max, "PBR_BLOOM_SMALL_MAX_PIXELS", 40000)) {
        // four lanes per pixel where a level is too small to fill the chip and goes through the general sampler (PBR_BLOOM_SMALL_MAX_PIXELS)
        kernel = a->upsample ? k_bloom_small<true> : k_bloom_small<false>; grid.y = rows;
    } else kernel = a->upsample ? k_bloom_pass<true> : k_bloom_pass<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    return launched();
}

extern "C" __attribute__((visibility("hidden"))) int pbrk_debug_sample_post(const void* texture, int w, int h, const void* coords, int count, void* out, void* stream) {
    PbrkTex2D t; t.data = texture; t.format = PBRK_FMT_RGBA16F; t.width = w; t.height = h;
    hipLaunchKernelGGL(k_debug_sample_post, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, t, (const float*)coords, count, (float4*)out);
    return launched();
}
