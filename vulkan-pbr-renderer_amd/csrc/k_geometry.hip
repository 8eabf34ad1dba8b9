// k_geometry.hip -- K13: the geometry pass, shaders/geometry_pass.glsl (render.cpp:1076-1115), as a compute rasteriser on K12's
// structure.  The rules live in geometry_core.h, the raster-job machinery shared with K12 (record, pixel box, draw
// lookup, counting, scan, fill, pre-filter, batch loop, launch sequence) in raster_bins.h; this file is what is K13's own:
//   * setup (one thread per source triangle): vertex stage, clip, fan, snap (geo_setup) -> one attribute record and up to six
//     coverage records (slots 6 t .. 6 t + 5; unused ones cover nothing), each counted into the tiles its pixel box touches;
//   * scan and fill: K12's, over the 6 n coverage records;
//   * tiles (one workgroup per 32 x 32 tile, 256 lanes, ONE WHOLE 2 x 2 QUAD PER LANE):
//       phase A  walk the tile's bin and the large list through LDS as K12 does; for every covered centre whose depth passes LESS
//                against the pixel's best so far (ties: the lower triangle number), run the alpha test and keep (depth, triangle);
//       phase B  shade each pixel's winner once and store the five colour targets and the depth.  Pixels nobody wins are not written.
//     No atomics touch a target.
//   * pbrk_mip_chain_rgba8: the mip chain of a material texture.
#include "geometry_core.h"
#include "raster_bins.h"

#include <hip/hip_fp16.h>

namespace {
constexpr int kFan = 6;                   // coverage records per source triangle (a triangle cut by five planes has at most 8 corners)
constexpr unsigned kNone = 0xFFFFFFFFu;

__device__ inline float sel4(const float* a, int q) { return q == 0 ? a[0] : q == 1 ? a[1] : q == 2 ? a[2] : a[3]; }
__device__ inline unsigned sel4(const unsigned* a, int q) { return q == 0 ? a[0] : q == 1 ? a[1] : q == 2 ? a[2] : a[3]; }

__global__ __launch_bounds__(kThreads) void k_geo_setup(PbrkGeometryArgs a, Layout L) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    bool rejected = false;
    char* scratch = (char*)a.scratch;
    if (t < a.tri_count) {
        const int di = find_draw(a.draws, a.draw_count, t);
        const PbrkGeoDraw& d = a.draws[di];
        const uint32_t* ix = d.indices + (size_t)d.first_index + 3 * (size_t)(t - d.first_tri);   // in range: checked at record time
        const float* v[3] = {nullptr, nullptr, nullptr};
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            const unsigned long long vi = (unsigned long long)ix[k] + d.vertex_offset;
            if (vi >= d.vertex_count) { ok = false; break; }
            v[k] = (const float*)((const char*)d.vertices + vi * 44u);
        }
        GeoCov cov[kFan];
        int n = 0;
        if (ok) {
            GeoAttr A;
            n = geo_setup(d, v[0], v[1], v[2], a.width, a.height, A, cov);
            if (n > 0) { A.draw = (uint32_t)di; ((GeoAttr*)(scratch + L.extra))[t] = A; }
        }
        rejected = !ok || n < 0;
        for (int k = 0; k < kFan; ++k) {
            TriRec r;                                                       // slots past the fan cover nothing
            r.pad = __uint_as_float(t);
            if (k < n) {
                r.x0 = cov[k].x[0]; r.y0 = cov[k].y[0]; r.x1 = cov[k].x[1]; r.y1 = cov[k].y[1]; r.x2 = cov[k].x[2]; r.y2 = cov[k].y[2];
                r.set_box(pixel_box(r.x0, r.y0, r.x1, r.y1, r.x2, r.y2, a.width, a.height));
            }
            store_rec(scratch, L, (size_t)kFan * t + k, r);
            if (!r.box().empty()) count_box(scratch, L, r.box(), kFan * t + k, false);
        }
    }
    const unsigned long long m = __ballot(rejected);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.rejected, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kThreads) void k_geo_tiles(PbrkGeometryArgs a, Layout L) {
    __shared__ int4 lds[kThreads * 4];                                      // 256 records, 16 KB
    __shared__ unsigned kept[kThreads];
    __shared__ unsigned nkept;
    const char* scratch = (const char*)a.scratch;
    const int qx = blockIdx.x * kTile + 2 * (int)(threadIdx.x & 15);        // this lane: the quad (qx .. qx + 1, qy .. qy + 1)
    const int qy = blockIdx.y * kTile + 2 * (int)(threadIdx.x >> 4);
    const int W = a.width, H = a.height;
    float bz[4];
    unsigned bt[4] = {kNone, kNone, kNone, kNone};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = qx + (q & 1), j = qy + (q >> 1);
        bz[q] = (i < W && j < H) ? a.depth[(size_t)j * W + i] : -1.0f;
    }
    const GeoAttr* attrs = (const GeoAttr*)(scratch + L.extra);
    const TriRec* sr = (const TriRec*)lds;
    // phase A: the winner does not depend on the order of the records
    walk_tile(scratch, L, lds, kept, &nkept, [&](unsigned k) {
        const TriRec& r = sr[k];
        const PixBox b = r.box();
        if (qy + 1 < b.y0 || qy > b.y1 || qx + 1 < b.x0 || qx > b.x1) return;
        GeoCov c;
        c.x[0] = r.x0; c.y[0] = r.y0; c.x[1] = r.x1; c.y[1] = r.y1; c.x[2] = r.x2; c.y[2] = r.y2;
        const unsigned src = __float_as_uint(r.pad);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = qx + (q & 1), jj = qy + (q >> 1);
            if (i >= W || jj >= H || i < b.x0 || i > b.x1 || jj < b.y0 || jj > b.y1 || !geo_covers(c, i, jj)) continue;
            const GeoAttr& A = attrs[src];
            double lam[3];
            float z;
            geo_lambda(A, i, jj, W, H, lam);
            if (!geo_depth(A, lam, &z)) continue;
            const float cz = sel4(bz, q);
            const unsigned ct = sel4(bt, q);
            if (!(z < cz || (z == cz && ct != kNone && src < ct))) continue;   // LESS; among this pass's fragments the lower triangle wins a tie
            GeoPix P;
            geo_pix(A, i, jj, W, H, P);
            if (geo_alpha(a.draws[A.draw], P) < 0.3f) continue;            // discard: neither wins nor writes
            if (q == 0) { bz[0] = z; bt[0] = src; } else if (q == 1) { bz[1] = z; bt[1] = src; }
            else if (q == 2) { bz[2] = z; bt[2] = src; } else { bz[3] = z; bt[3] = src; }
        }
    });
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
        const unsigned src = sel4(bt, q);
        if (src == kNone) continue;                                         // in-range by construction: only in-range pixels get a winner
        const int i = qx + (q & 1), j = qy + (q >> 1);
        const GeoAttr& A = attrs[src];
        GeoPix P;
        GeoOut o;
        geo_pix(A, i, j, W, H, P);
        geo_shade(a.draws[A.draw], A, P, i, j, W, H, o);
        const size_t p = (size_t)j * W + i;
        ((uchar4*)a.color[0])[p] = make_uchar4(o.base[0], o.base[1], o.base[2], o.base[3]);
        ((uchar4*)a.color[1])[p] = make_uchar4(o.nrm[0], o.nrm[1], o.nrm[2], o.nrm[3]);
        ((uchar4*)a.color[2])[p] = make_uchar4(o.orm[0], o.orm[1], o.orm[2], o.orm[3]);
        ((uchar4*)a.color[3])[p] = make_uchar4(o.emi[0], o.emi[1], o.emi[2], o.emi[3]);
        ((__half2*)a.velocity)[p] = __halves2half2(__float2half_rn(o.vel[0]), __float2half_rn(o.vel[1]));
        a.depth[p] = sel4(bz, q);
    }
}

// one level of an RGBA8UN chain: (w, h) is the size of the level written
__global__ __launch_bounds__(kThreads) void k_mip_rgba8(const uchar4* src, uchar4* dst, int w, int h) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= w * h) return;
    const int x = p % w, y = p / w, sw = 2 * w;
    const uchar4 t00 = src[(size_t)(2 * y) * sw + 2 * x], t10 = src[(size_t)(2 * y) * sw + 2 * x + 1];
    const uchar4 t01 = src[(size_t)(2 * y + 1) * sw + 2 * x], t11 = src[(size_t)(2 * y + 1) * sw + 2 * x + 1];
    auto box = [](unsigned char a, unsigned char b, unsigned char c, unsigned char d) {
        const float s = (((float)a / 255.0f + (float)b / 255.0f) + ((float)c / 255.0f + (float)d / 255.0f)) * 0.25f;
        return (unsigned char)rintf(255.0f * s);
    };
    dst[p] = make_uchar4(box(t00.x, t10.x, t01.x, t11.x), box(t00.y, t10.y, t01.y, t11.y), box(t00.z, t10.z, t01.z, t11.z), box(t00.w, t10.w, t01.w, t11.w));
}

bool args_ok(const PbrkGeometryArgs* a) {
    return a && a->draws && a->color[0] && a->color[1] && a->color[2] && a->color[3] && a->velocity && a->depth && a->scratch && a->rejected &&
           a->draw_count > 0 && dims_ok(a->width, a->height) && a->tri_count <= (1u << 26);
}
Layout geo_layout(uint32_t n, int W, int H) { return raster_layout(kFan * n, W, H, (size_t)n * sizeof(GeoAttr)); }
}  // namespace

extern "C" size_t pbrk_geometry_scratch_bytes(uint32_t tri_count, int width, int height) {
    if (width <= 0 || height <= 0 || tri_count > (1u << 26)) return 0;
    return geo_layout(tri_count, width, height).total;
}

extern "C" int pbrk_geometry_setup(const PbrkGeometryArgs* a, void* stream) {
    if (!args_ok(a)) return PBRK_E_ARG;
    if (a->tri_count == 0) return PBRK_OK;
    const Layout L = geo_layout(a->tri_count, a->width, a->height);
    return launch_binning(k_geo_setup, *a, L, kFan * a->tri_count, (hipStream_t)stream) ? PBRK_OK : PBRK_E_LAUNCH;
}

extern "C" int pbrk_geometry_tiles(const PbrkGeometryArgs* a, void* stream) {
    if (!args_ok(a)) return PBRK_E_ARG;
    if (a->tri_count == 0) return PBRK_OK;
    const Layout L = geo_layout(a->tri_count, a->width, a->height);
    hipLaunchKernelGGL(k_geo_tiles, dim3(L.tx, L.ty), dim3(kThreads), 0, (hipStream_t)stream, *a, L);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}

extern "C" int pbrk_mip_chain_rgba8(void* pyramid, int width, int height, int levels, void* stream) {
    if (!pyramid || width <= 0 || height <= 0 || levels < 1 || (width & (width - 1)) || (height & (height - 1))) return PBRK_E_ARG;
    char* base = (char*)pyramid;
    int w = width, h = height;
    for (int l = 1; l < levels; ++l) {
        if (w < 2 || h < 2) return PBRK_E_ARG;
        char* next = base + (size_t)w * h * 4;
        w >>= 1; h >>= 1;
        hipLaunchKernelGGL(k_mip_rgba8, dim3((w * h + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, (const uchar4*)base, (uchar4*)next, w, h);
        base = next;
    }
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}
