// geometry_core.h -- the per-triangle and per-pixel rules of the geometry pass (K13), written once for the device
// kernels of k_geometry.hip and for a host compiler: every function is plain scalar C++ without FMA contraction, so a CPU build
// of this header evaluates the contract exactly as the kernels do (all but pow22, which is the hardware log2 / exp2 on the GPU).
// Cited shader lines: geometry_pass.glsl of the reference renderer.
#pragma once
#include "pbr_kernels.h"

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GEO_FN __host__ __device__ __forceinline__
#else
#define GEO_FN static inline
#endif

struct GeoAttr {                  // one per source triangle: what interpolation needs (all of it from the ORIGINAL triangle)
    double adj[9];                // rows of the adjugate of [a b c], a/b/c = (x_c, y_c, w) of vertex 0/1/2: b x c, c x a, a x b
    float z[3], w[3];             // clip-space z and w
    uint32_t draw, valid;         // valid = determinant != 0
    float uv[3][2], pos[3][3], nrm[3][3], cs[3][2], old[3][3];   // cs = jittered clip x, y; old = old clip x, y, w
};
struct GeoCov { int x[3], y[3]; };                   // one fan triangle, snapped to 1/256 px, front-facing (area < 0)
// a pixel's interpolants and their fine derivatives: the triangle evaluated at the pixel's own centre and at the horizontal and the
// vertical neighbour centre of its 2x2 quad (quads start at even coordinates); d/dx = value at odd x minus value at even x
struct GeoPix { float uv[2], pos[3], dxu[2], dyu[2], dxp[3], dyp[3]; };
struct GeoOut { uint8_t base[4], nrm[4], orm[4], emi[4]; float vel[2]; };

GEO_FN uint32_t geo_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
GEO_FN float geo_from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
GEO_FN bool geo_finite(float x) { return fabsf(x) <= FLT_MAX; }

// ---- vertex stage (geometry_pass.glsl:109-113): M (p, 1) per row as ((m0 x + m1 y) + m2 z) + m3, then xy += jitter * w ----
GEO_FN void geo_vertex(const float* m, const float* jit, const float* p, float c[4]) {
    const float x = p[0], y = p[1], z = p[2];
    for (int r = 0; r < 4; ++r) c[r] = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r];
    c[0] = c[0] + jit[0] * c[3];
    c[1] = c[1] + jit[1] * c[3];
}

// clip planes in their fixed order: z >= 0, x >= -64 w, x <= 64 w, y >= -64 w, y <= 64 w
GEO_FN float geo_plane(int p, const float* c) {
    const float g = 64.0f * c[3];
    switch (p) {
    case 0: return c[2];
    case 1: return g + c[0];
    case 2: return g - c[0];
    case 3: return g + c[1];
    default: return g - c[1];
    }
}

// K12 rule 4: divide, viewport, guard band, snap to 1/256 px
GEO_FN bool geo_snap(const float* c, int W, int H, int* X, int* Y) {
    const float hw = (float)W * 0.5f, hh = (float)H * 0.5f;
    const float xd = c[0] / c[3], yd = c[1] / c[3];
    const float xf = hw * xd + hw, yf = hh * yd + hh;
    if (!(fabsf(xf) <= 2097152.0f) || !(fabsf(yf) <= 2097152.0f)) return false;
    *X = (int)rintf(xf * 256.0f); *Y = (int)rintf(yf * 256.0f);
    return true;
}

// One source triangle (v0, v1, v2: 11 floats each, render.h Vertex).  Returns -1 when it is rejected (counted), else the number
// of coverage triangles written to cov (0 .. 6); A is filled whenever the result is > 0.
GEO_FN int geo_setup(const PbrkGeoDraw& d, const float* v0, const float* v1, const float* v2, int W, int H, GeoAttr& A, GeoCov* cov) {
    const float* v[3] = {v0, v1, v2};
    float c[3][4];
    for (int k = 0; k < 3; ++k) {
        float o[4];
        geo_vertex(d.m, d.jitter, v[k], c[k]);
        geo_vertex(d.m_old, d.jitter_prev, v[k], o);
        if (!geo_finite(c[k][0]) || !geo_finite(c[k][1]) || !geo_finite(c[k][2]) || !geo_finite(c[k][3])) return -1;
        A.z[k] = c[k][2]; A.w[k] = c[k][3];
        A.cs[k][0] = c[k][0]; A.cs[k][1] = c[k][1];
        A.old[k][0] = o[0]; A.old[k][1] = o[1]; A.old[k][2] = o[3];
        for (int e = 0; e < 3; ++e) { A.pos[k][e] = v[k][e]; A.nrm[k][e] = v[k][3 + e]; }
        A.uv[k][0] = v[k][9]; A.uv[k][1] = v[k][10];
    }
    A.draw = 0;
    {
        const double ax = c[0][0], ay = c[0][1], aw = c[0][3], bx = c[1][0], by = c[1][1], bw = c[1][3], cx = c[2][0], cy = c[2][1], cw = c[2][3];
        A.adj[0] = by * cw - bw * cy; A.adj[1] = bw * cx - bx * cw; A.adj[2] = bx * cy - by * cx;     // b x c
        A.adj[3] = cy * aw - cw * ay; A.adj[4] = cw * ax - cx * aw; A.adj[5] = cx * ay - cy * ax;     // c x a
        A.adj[6] = ay * bw - aw * by; A.adj[7] = aw * bx - ax * bw; A.adj[8] = ax * by - ay * bx;     // a x b
        const double det = (ax * A.adj[0] + ay * A.adj[1]) + aw * A.adj[2];
        A.valid = det != 0.0;
        if (!A.valid) return 0;
    }
    bool all_in = true;
    for (int p = 0; p < 5; ++p) {
        int out = 0;
        for (int k = 0; k < 3; ++k) out += !(geo_plane(p, c[k]) >= 0.0f);
        if (out == 3) return 0;                                               // entirely behind one plane: dropped silently
        if (out) all_in = false;
    }
    float P[9][4], Q[9][4];
    int n = 3;
    for (int k = 0; k < 3; ++k) for (int e = 0; e < 4; ++e) P[k][e] = c[k][e];
    if (!all_in) {                                                            // Sutherland-Hodgman, plane after plane
        for (int p = 0; p < 5 && n > 0; ++p) {
            int m = 0;
            for (int e = 0; e < n; ++e) {
                const float* a = P[e];
                const float* b = P[e + 1 == n ? 0 : e + 1];
                const float da = geo_plane(p, a), db = geo_plane(p, b);
                const bool ia = da >= 0.0f, ib = db >= 0.0f;
                if (ia && m < 9) { for (int q = 0; q < 4; ++q) Q[m][q] = a[q]; ++m; }
                if (ia != ib && m < 9) {
                    const float t = da / (da - db);
                    for (int q = 0; q < 4; ++q) Q[m][q] = a[q] + t * (b[q] - a[q]);
                    ++m;
                }
            }
            n = m;
            for (int e = 0; e < n; ++e) for (int q = 0; q < 4; ++q) P[e][q] = Q[e][q];
        }
        if (n < 3) return 0;
        if (n > 8) n = 8;
    }
    int X[8], Y[8];
    for (int e = 0; e < n; ++e) if (!geo_snap(P[e], W, H, &X[e], &Y[e])) return -1;
    int count = 0;
    for (int e = 1; e + 1 < n; ++e) {
        const long long x0 = X[0], y0 = Y[0], x1 = X[e], y1 = Y[e], x2 = X[e + 1], y2 = Y[e + 1];
        const long long area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
        if (area >= 0) continue;                                              // GPU_CullMode_DrawCCW: negative area (y down) is drawn
        GeoCov& o = cov[count++];
        o.x[0] = X[0]; o.y[0] = Y[0]; o.x[1] = X[e]; o.y[1] = Y[e]; o.x[2] = X[e + 1]; o.y[2] = Y[e + 1];
    }
    return count;
}

// K12's coverage rule for a triangle of negative area: exact edge functions, inside positive after the sign flip, top-left rule
GEO_FN bool geo_covers(const GeoCov& t, int i, int j) {
    const long long Px = 256LL * i + 128, Py = 256LL * j + 128;
    for (int k = 0; k < 3; ++k) {
        const int a = k == 2 ? 0 : k + 1, b = a == 2 ? 0 : a + 1;             // edges v1->v2, v2->v0, v0->v1
        const long long ax = t.x[a], ay = t.y[a], bx = t.x[b], by = t.y[b];
        const long long e = -((bx - ax) * (Py - ay) - (by - ay) * (Px - ax));
        const long long na = (by - ay), nb = -(bx - ax);                      // inward normal (A, B) of the flipped edge
        if (e < 0) return false;
        if (e == 0 && !(na > 0 || (na == 0 && nb > 0))) return false;
    }
    return true;
}

// ---- interpolation: l = adj (xn, yn, 1), lambda = l / (l0 + l1 + l2), all fp64 ----
GEO_FN void geo_lambda(const GeoAttr& A, int i, int j, int W, int H, double lam[3]) {
    const double xn = (double)(2 * i + 1) / (double)W - 1.0, yn = (double)(2 * j + 1) / (double)H - 1.0;
    const double l0 = (A.adj[0] * xn + A.adj[1] * yn) + A.adj[2];
    const double l1 = (A.adj[3] * xn + A.adj[4] * yn) + A.adj[5];
    const double l2 = (A.adj[6] * xn + A.adj[7] * yn) + A.adj[8];
    const double s = (l0 + l1) + l2;
    lam[0] = l0 / s; lam[1] = l1 / s; lam[2] = l2 / s;
}
GEO_FN float geo_interp(const double lam[3], float a0, float a1, float a2) {
    return (float)((lam[0] * (double)a0 + lam[1] * (double)a1) + lam[2] * (double)a2);
}
GEO_FN bool geo_depth(const GeoAttr& A, const double lam[3], float* z) {
    const double num = (lam[0] * (double)A.z[0] + lam[1] * (double)A.z[1]) + lam[2] * (double)A.z[2];
    const double den = (lam[0] * (double)A.w[0] + lam[1] * (double)A.w[1]) + lam[2] * (double)A.w[2];
    float zf = (float)(num / den);
    if (!(zf >= 0.0f && zf <= 1.0f)) return false;
    if (zf == 0.0f) zf = 0.0f;                                                // -0 -> +0
    *z = zf;
    return true;
}
GEO_FN void geo_pix(const GeoAttr& A, int i, int j, int W, int H, GeoPix& P) {
    double lam[3];
    float ux[2], px[3], uy[2], py[3];
    geo_lambda(A, i, j, W, H, lam);
    for (int e = 0; e < 2; ++e) P.uv[e] = geo_interp(lam, A.uv[0][e], A.uv[1][e], A.uv[2][e]);
    for (int e = 0; e < 3; ++e) P.pos[e] = geo_interp(lam, A.pos[0][e], A.pos[1][e], A.pos[2][e]);
    geo_lambda(A, i ^ 1, j, W, H, lam);
    for (int e = 0; e < 2; ++e) ux[e] = geo_interp(lam, A.uv[0][e], A.uv[1][e], A.uv[2][e]);
    for (int e = 0; e < 3; ++e) px[e] = geo_interp(lam, A.pos[0][e], A.pos[1][e], A.pos[2][e]);
    geo_lambda(A, i, j ^ 1, W, H, lam);
    for (int e = 0; e < 2; ++e) uy[e] = geo_interp(lam, A.uv[0][e], A.uv[1][e], A.uv[2][e]);
    for (int e = 0; e < 3; ++e) py[e] = geo_interp(lam, A.pos[0][e], A.pos[1][e], A.pos[2][e]);
    const bool ox = i & 1, oy = j & 1;
    for (int e = 0; e < 2; ++e) { P.dxu[e] = ox ? P.uv[e] - ux[e] : ux[e] - P.uv[e]; P.dyu[e] = oy ? P.uv[e] - uy[e] : uy[e] - P.uv[e]; }
    for (int e = 0; e < 3; ++e) { P.dxp[e] = ox ? P.pos[e] - px[e] : px[e] - P.pos[e]; P.dyp[e] = oy ? P.pos[e] - py[e] : py[e] - P.pos[e]; }
}

// ---- texture(): linear min / mag / mip, repeat ----
// log2 of a finite x > 1: the exponent exactly, a degree-4 polynomial in the mantissa (|error| < 2^-9 level over every mantissa:
// about 1.0e-4, tests/test_geometry_raster_cpu.py)
#define GEO_LOG2_C1 1.4390145540237427f
#define GEO_LOG2_C2 -0.6799435615539551f
#define GEO_LOG2_C3 0.32559481263160706f
#define GEO_LOG2_C4 -0.08476819097995758f
GEO_FN float geo_log2(float x) {
    const uint32_t b = geo_bits(x);
    const int e = (int)(b >> 23) - 127;
    const float t = geo_from_bits((b & 0x7FFFFFu) | 0x3F800000u) - 1.0f;
    const float p = t * (GEO_LOG2_C1 + t * (GEO_LOG2_C2 + t * (GEO_LOG2_C3 + t * GEO_LOG2_C4)));
    return (float)e + p;
}
GEO_FN float geo_snap256(float x) { return floorf(x * 256.0f + 0.5f) * (1.0f / 256.0f); }
// level of detail from the quad's uv differences, clamped and snapped to 1/256 level; < 0: non-finite footprint
GEO_FN float geo_lod(const PbrkGeoTex& t, float dudx, float dvdx, float dudy, float dvdy) {
    const float ax = dudx * (float)t.width, bx = dvdx * (float)t.height, ay = dudy * (float)t.width, by = dvdy * (float)t.height;
    const float lx = ax * ax + bx * bx, ly = ay * ay + by * by;
    if (!(lx <= FLT_MAX) || !(ly <= FLT_MAX)) return -1.0f;
    const float rho = sqrtf(lx > ly ? lx : ly);
    float lod = rho > 1.0f ? geo_log2(rho) : 0.0f;
    const float top = (float)(t.levels - 1);
    if (lod > top) lod = top;
    return geo_snap256(lod);
}
GEO_FN void geo_bilinear(const PbrkGeoTex& t, int level, float u, float v, float out[4]) {
    size_t off = 0;
    int w = t.width, h = t.height;
    for (int l = 0; l < level; ++l) { off += (size_t)w * h * 4; w = w > 1 ? w >> 1 : 1; h = h > 1 ? h >> 1 : 1; }
    const uint8_t* px = (const uint8_t*)t.texels + off;
    const float uw = u - floorf(u), vw = v - floorf(v);                      // repeat: [0, 1] before any conversion to int
    const float x = geo_snap256(uw * (float)w - 0.5f), y = geo_snap256(vw * (float)h - 0.5f);
    const float fx = floorf(x), fy = floorf(y);
    const float a = x - fx, b = y - fy;
    int i0 = (int)fx, j0 = (int)fy;                                           // in [-1, w] / [-1, h]
    i0 = i0 < 0 ? i0 + w : (i0 >= w ? i0 - w : i0);
    j0 = j0 < 0 ? j0 + h : (j0 >= h ? j0 - h : j0);
    const int i1 = i0 + 1 >= w ? 0 : i0 + 1, j1 = j0 + 1 >= h ? 0 : j0 + 1;
    const uint8_t* t00 = px + ((size_t)j0 * w + i0) * 4;
    const uint8_t* t10 = px + ((size_t)j0 * w + i1) * 4;
    const uint8_t* t01 = px + ((size_t)j1 * w + i0) * 4;
    const uint8_t* t11 = px + ((size_t)j1 * w + i1) * 4;
    for (int c = 0; c < 4; ++c) {
        const float c00 = (float)t00[c] / 255.0f, c10 = (float)t10[c] / 255.0f, c01 = (float)t01[c] / 255.0f, c11 = (float)t11[c] / 255.0f;
        const float top = c00 + a * (c10 - c00), bot = c01 + a * (c11 - c01);
        out[c] = top + b * (bot - top);
    }
}
// texture(sampler2D(t, SAMPLER_LINEAR_WRAP), uv)
GEO_FN void geo_texture(const PbrkGeoTex& t, const GeoPix& P, float out[4]) {
    float u = P.uv[0], v = P.uv[1];
    float lod = geo_lod(t, P.dxu[0], P.dxu[1], P.dyu[0], P.dyu[1]);
    if (lod < 0.0f || !geo_finite(u) || !geo_finite(v)) { u = 0.0f; v = 0.0f; lod = (float)(t.levels - 1); }   // coarsest level, coordinate 0
    const int l0 = (int)lod;
    const float f = lod - (float)l0;
    geo_bilinear(t, l0, u, v, out);
    if (f > 0.0f) {                                                           // then l0 + 1 <= levels - 1
        float c1[4];
        geo_bilinear(t, l0 + 1, u, v, c1);
        for (int c = 0; c < 4; ++c) out[c] = out[c] + f * (c1[c] - out[c]);
    }
}

GEO_FN float geo_pow22(float x) {                                             // pow(x, 2.2) as K9 computes its pow
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(2.2f * __builtin_amdgcn_logf(x));
#else
    return exp2f(2.2f * log2f(x));
#endif
}
GEO_FN uint8_t geo_unorm8(float x) {
    float c = x;
    if (!(c >= 0.0f)) c = 0.0f;                                               // NaN -> 0
    if (c > 1.0f) c = 1.0f;
    return (uint8_t)rintf(255.0f * c);
}
GEO_FN float geo_dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
GEO_FN void geo_normalize3(float* a) {
    const float len = sqrtf(geo_dot3(a, a));
    a[0] = a[0] / len; a[1] = a[1] / len; a[2] = a[2] / len;
}
GEO_FN void geo_cross3(const float* a, const float* b, float* r) {
    r[0] = a[1] * b[2] - b[1] * a[2]; r[1] = a[2] * b[0] - b[2] * a[0]; r[2] = a[0] * b[1] - b[0] * a[1];
}

// the alpha the discard of geometry_pass.glsl:258-259 tests
GEO_FN float geo_alpha(const PbrkGeoDraw& d, const GeoPix& P) {
    float bc[4];
    geo_texture(d.tex[0], P, bc);
    return bc[3];
}

// geometry_pass.glsl:258-320 for pixel (i, j).  The lines 267, 270, 271 (V, T, VdotN) feed nothing and are left out.
GEO_FN void geo_shade(const PbrkGeoDraw& d, const GeoAttr& A, const GeoPix& P, int i, int j, int W, int H, GeoOut& o) {
    float bc[4], orm[4], emi[4], tn[4];
    geo_texture(d.tex[0], P, bc);
    for (int c = 0; c < 4; ++c) o.base[c] = geo_unorm8(geo_pow22(bc[c]));
    geo_texture(d.tex[2], P, orm);
    geo_texture(d.tex[3], P, emi);
    for (int c = 0; c < 3; ++c) { o.orm[c] = geo_unorm8(orm[c]); o.emi[c] = geo_unorm8(emi[c]); }
    o.orm[3] = 255; o.emi[3] = 255;
    double lam[3];
    geo_lambda(A, i, j, W, H, lam);
    float N[3];
    for (int e = 0; e < 3; ++e) N[e] = geo_interp(lam, A.nrm[0][e], A.nrm[1][e], A.nrm[2][e]);
    geo_normalize3(N);
    geo_texture(d.tex[1], P, tn);
    float ts[3];
    ts[0] = tn[0] * 2.0f - 1.0f; ts[1] = tn[1] * 2.0f - 1.0f;
    ts[2] = sqrtf(1.0f - (ts[0] * ts[0] + ts[1] * ts[1]));
    const float* dxu = P.dxu; const float* dyu = P.dyu; const float* dxp = P.dxp; const float* dyp = P.dyp;
    float T[3], B[3], den[3];
    if (dxu[0] * dyu[1] - dxu[1] * dyu[0] < 0.0f) {
        for (int e = 0; e < 3; ++e) den[e] = dxp[e] * dyu[0] - dyp[e] * dxu[0];
        const float nd = geo_dot3(N, den);
        for (int e = 0; e < 3; ++e) B[e] = den[e] - N[e] * nd;
        geo_normalize3(B);
        geo_cross3(B, N, T);
    } else {
        for (int e = 0; e < 3; ++e) den[e] = dxp[e] * dyu[1] - dyp[e] * dxu[1];
        const float nd = geo_dot3(N, den);
        for (int e = 0; e < 3; ++e) T[e] = den[e] - N[e] * nd;
        geo_normalize3(T);
        geo_cross3(T, N, B);
    }
    for (int e = 0; e < 3; ++e) {
        const float n = (T[e] * ts[0] + B[e] * ts[1]) + N[e] * ts[2];         // TBN * tangent_space_normal
        o.nrm[e] = geo_unorm8(n * 0.5f + 0.5f);
    }
    o.nrm[3] = 255;
    const float cx = geo_interp(lam, A.cs[0][0], A.cs[1][0], A.cs[2][0]), cy = geo_interp(lam, A.cs[0][1], A.cs[1][1], A.cs[2][1]);
    const float cw = geo_interp(lam, A.w[0], A.w[1], A.w[2]);
    const float ox = geo_interp(lam, A.old[0][0], A.old[1][0], A.old[2][0]), oy = geo_interp(lam, A.old[0][1], A.old[1][1], A.old[2][1]);
    const float ow = geo_interp(lam, A.old[0][2], A.old[1][2], A.old[2][2]);
    o.vel[0] = (cx / cw - d.jitter[0]) - (ox / ow - d.jitter_prev[0]);
    o.vel[1] = (cy / cw - d.jitter[1]) - (oy / ow - d.jitter_prev[1]);
}
