// voxelize_core.h -- the per-triangle and per-fragment rules of the voxelise pass (K14), written once for the device
// kernels of k_voxelize.hip and for a host compiler, on top of geometry_core.h (texture(), cross, dot) and shadow_core.h (the shadow
// tap): plain scalar C++ without FMA contraction, so a CPU build evaluates the contract exactly as the kernels do.
// Cited shader lines: lightgrid_voxelize.glsl of the reference renderer.
#pragma once
#include "geometry_core.h"
#include "shadow_core.h"

struct VoxTri {                   // one triangle after the vertex stage
    int X[3], Y[3];               // snapped target coordinates, 1/256 px
    int box[4];                   // conservative pixel box i0, j0, i1, j1, clamped to the target; i0 > i1: empty
    double inv;                   // 1 / (E0 + E1 + E2)
    float p[3][3], uv[3][2], n[3];   // world positions, texture coordinates, normalised face normal
    float scale;
};

GEO_FN float vox_max(float x, float y) { return x < y ? y : x; }              // GLSL max: y if x < y, else x

// Vertex stage and snap of triangle `local_tri` of draw d (:37-78).  1: may produce fragments; 0: zero area after snapping or a box
// outside the target (nothing drawn); -1: rejected (counted).
GEO_FN int vox_setup(const PbrkVoxDraw& d, uint32_t local_tri, int N, VoxTri& T) {
    const unsigned long long base = (unsigned long long)d.first_vertex + 3ull * local_tri, nf = d.vertex_floats;
    for (int k = 0; k < 3; ++k) {
        const unsigned long long o = 11ull * d.indices[base + k];
        if (o + 2 >= nf) return -1;                                           // a position past the end of SSBO0
        for (int e = 0; e < 3; ++e) T.p[k][e] = d.vertices[o + e];
        if (!geo_finite(T.p[k][0]) || !geo_finite(T.p[k][1]) || !geo_finite(T.p[k][2])) return -1;
        const unsigned long long u = (base + k) * 11ull + 9ull;              // :54 reads the uv of vertex gl_VertexIndex, not of v_k
        T.uv[k][0] = u < nf ? d.vertices[u] : 0.0f;
        T.uv[k][1] = u + 1 < nf ? d.vertices[u + 1] : 0.0f;
    }
    float e1[3], e2[3], nrm[3];
    for (int e = 0; e < 3; ++e) { e1[e] = T.p[1][e] - T.p[0][e]; e2[e] = T.p[2][e] - T.p[0][e]; }
    geo_cross3(e1, e2, nrm);
    const float ax = fabsf(nrm[0]), ay = fabsf(nrm[1]), az = fabsf(nrm[2]);
    const float mx = vox_max(vox_max(ax, ay), az);
    const int axis = mx == ax ? 0 : (mx == ay ? 1 : 2);                       // :63-69
    const float hn = (float)N * 0.5f;
    T.scale = d.scale;
    for (int k = 0; k < 3; ++k) {
        const float g[3] = {T.p[k][0] * d.scale, T.p[k][1] * d.scale, T.p[k][2] * d.scale};
        const float x = axis == 0 ? g[1] : (axis == 1 ? g[2] : g[0]);        // yzx / zxy / xyz
        const float y = axis == 0 ? g[2] : (axis == 1 ? g[0] : g[1]);
        const float z = (axis == 0 ? g[0] : (axis == 1 ? g[1] : g[2])) * 0.5f + 0.5f;
        const float xf = hn * x + hn, yf = hn * y + hn;
        if (!(fabsf(xf) <= 2097152.0f) || !(fabsf(yf) <= 2097152.0f) || !geo_finite(z)) return -1;
        T.X[k] = (int)rintf(xf * 256.0f); T.Y[k] = (int)rintf(yf * 256.0f);
    }
    const long long x0 = T.X[0], y0 = T.Y[0], x1 = T.X[1], y1 = T.Y[1], x2 = T.X[2], y2 = T.Y[2];
    const long long area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
    if (area == 0) return 0;
    T.inv = 1.0 / (double)area;
    const long long mnx = x0 < x1 ? (x0 < x2 ? x0 : x2) : (x1 < x2 ? x1 : x2), mxx = x0 > x1 ? (x0 > x2 ? x0 : x2) : (x1 > x2 ? x1 : x2);
    const long long mny = y0 < y1 ? (y0 < y2 ? y0 : y2) : (y1 < y2 ? y1 : y2), mxy = y0 > y1 ? (y0 > y2 ? y0 : y2) : (y1 > y2 ? y1 : y2);
    // pixels whose closed square [256 i, 256 i + 256] meets the closed bounding box
    long long i0 = (mnx - 1) >> 8, i1 = mxx >> 8, j0 = (mny - 1) >> 8, j1 = mxy >> 8;
    if (i0 < 0) i0 = 0;
    if (j0 < 0) j0 = 0;
    if (i1 > N - 1) i1 = N - 1;
    if (j1 > N - 1) j1 = N - 1;
    if (i0 > i1 || j0 > j1) return 0;
    T.box[0] = (int)i0; T.box[1] = (int)j0; T.box[2] = (int)i1; T.box[3] = (int)j1;
    const float len = sqrtf(geo_dot3(nrm, nrm));
    for (int e = 0; e < 3; ++e) T.n[e] = nrm[e] / len;
    return 1;
}

// Does pixel (i, j) produce a fragment?  Its closed square must meet the closed snapped triangle: inside the box, and for every edge
// (inside positive for either winding) the largest of the four corner values -- the corner the edge's gradient points to -- is >= 0.
GEO_FN bool vox_covers(const VoxTri& T, int i, int j) {
    if (i < T.box[0] || i > T.box[2] || j < T.box[1] || j > T.box[3]) return false;
    const long long sg = T.inv > 0.0 ? 1 : -1;
    const long long lo_x = 256LL * i, hi_x = lo_x + 256, lo_y = 256LL * j, hi_y = lo_y + 256;
    for (int k = 0; k < 3; ++k) {
        const int a = k == 2 ? 0 : k + 1, b = a == 2 ? 0 : a + 1;             // edges v1->v2, v2->v0, v0->v1
        const long long ax = T.X[a], ay = T.Y[a], bx = T.X[b], by = T.Y[b];
        const long long A = -(by - ay) * sg, B = (bx - ax) * sg;
        const long long Px = A > 0 ? hi_x : lo_x, Py = B > 0 ? hi_y : lo_y;
        if (sg * ((bx - ax) * (Py - ay) - (by - ay) * (Px - ax)) < 0) return false;
    }
    return true;
}

// K12 rule 5 at the centre of pixel (i, j), which may lie outside the triangle: exact integer edge values, fp64, one rounding
GEO_FN void vox_edges(const VoxTri& T, int i, int j, double* e1, double* e2) {
    const long long Px = 256LL * i + 128, Py = 256LL * j + 128;
    const long long x0 = T.X[0], y0 = T.Y[0], x1 = T.X[1], y1 = T.Y[1], x2 = T.X[2], y2 = T.Y[2];
    *e1 = (double)((x0 - x2) * (Py - y2) - (y0 - y2) * (Px - x2));
    *e2 = (double)((x1 - x0) * (Py - y0) - (y1 - y0) * (Px - x0));
}
GEO_FN float vox_interp(double e1, double e2, double inv, float a0, float a1, float a2) {
    return (float)((double)a0 + (e1 * ((double)a1 - (double)a0) + e2 * ((double)a2 - (double)a0)) * inv);
}

// The voxel the fragment of pixel (i, j) addresses (:123-125); false when it lies outside the grid.  ivec3() truncates toward zero, so
// a product in (-1, 0) lands in voxel 0; the range is tested on the float, before any conversion.
GEO_FN bool vox_coord(const VoxTri& T, int i, int j, int N, int c[3]) {
    double e1, e2;
    vox_edges(T, i, j, &e1, &e2);
    for (int e = 0; e < 3; ++e) {
        const float ndc = vox_interp(e1, e2, T.inv, T.p[0][e] * T.scale, T.p[1][e] * T.scale, T.p[2][e] * T.scale);
        const float q = (ndc * 0.5f + 0.5f) * (float)N;
        if (!(q > -1.0f && q < (float)N)) return false;
        c[e] = (int)q;
    }
    return true;
}

// The fragment stage (:100-128) of pixel (i, j): rgb of the stored value (alpha is 1)
GEO_FN void vox_shade(const PbrkVoxDraw& d, const VoxTri& T, int i, int j, float out[3]) {
    double e1, e2;
    float ws[3];
    GeoPix P;
    vox_edges(T, i, j, &e1, &e2);
    for (int e = 0; e < 3; ++e) ws[e] = vox_interp(e1, e2, T.inv, T.p[0][e], T.p[1][e], T.p[2][e]);
    for (int e = 0; e < 2; ++e) P.uv[e] = vox_interp(e1, e2, T.inv, T.uv[0][e], T.uv[1][e], T.uv[2][e]);
    vox_edges(T, i ^ 1, j, &e1, &e2);                                         // K13 rule 7: fine derivatives inside the 2 x 2 quad
    for (int e = 0; e < 2; ++e) {
        const float ux = vox_interp(e1, e2, T.inv, T.uv[0][e], T.uv[1][e], T.uv[2][e]);
        P.dxu[e] = (i & 1) ? P.uv[e] - ux : ux - P.uv[e];
    }
    vox_edges(T, i, j ^ 1, &e1, &e2);
    for (int e = 0; e < 2; ++e) {
        const float uy = vox_interp(e1, e2, T.inv, T.uv[0][e], T.uv[1][e], T.uv[2][e]);
        P.dyu[e] = (j & 1) ? P.uv[e] - uy : uy - P.uv[e];
    }
    const float* m = d.sun;
    float s[3];
    for (int r = 0; r < 3; ++r) s[r] = ((m[r] * ws[0] + m[4 + r] * ws[1]) + m[8 + r] * ws[2]) + m[12 + r];
    const float px = 1.0f / 2048.0f;
    const float su = (s[0] * 0.5f + 0.5f) + px, sv = (s[1] * 0.5f + 0.5f) + px, sz = s[2] - 0.001f;
    const float shadow = shadow_sample(d.sun_depth, d.sun_w, d.sun_h, su, sv, sz);
    const float L[3] = {-d.sun_dir[0], -d.sun_dir[1], -d.sun_dir[2]};
    const float LdotN = vox_max(geo_dot3(L, T.n), 0.0f);
    float bc[4], em[4];
    geo_texture(d.tex[0], P, bc);
    geo_texture(d.tex[1], P, em);
    const float sun[3] = {5.0f, 5.0f * 0.9f, 5.0f * 0.7f};
    for (int c = 0; c < 3; ++c) out[c] = em[c] + ((shadow * bc[c]) * LdotN) * sun[c];
}
