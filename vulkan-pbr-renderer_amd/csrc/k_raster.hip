// k_raster.hip -- K12 (N5): the sun depth pass, shaders/sun_depth_pass.glsl (render.cpp:993-1020), as a compute rasteriser.
//
// The pass has one matrix product per vertex, no fragment output, no culling, no blending: a LESS depth test and a depth write
// into a 2048^2 D32F target.  The result is a per-pixel minimum over every covered fragment, which does not depend on triangle
// order, so all draws of one render-pass instance are ONE job and the rules of DESIGN.md K12 are met bit for bit:
//   * setup (one thread per triangle): fetch the three indices, skip the triangle when a vertex index is past the vertex buffer,
//     transform in fp32 (m0 x + m1 y + m2 z + m3, no FMA: -ffp-contract=off), divide by w, viewport, reject what is not finite
//     or outside +-2^21 px (counted), snap to 1/256 px, write a 64-B record (snapped vertices, z0, z1-z0, z2-z0 and 1/area in
//     fp64, clamped pixel box) and count the record into every 32 x 32-pixel tile its box touches -- or, when that is more than
//     kMaxTiles tiles, append it to one "large" list;
//   * scan: exclusive prefix of the per-tile counts (one workgroup); fill: each binned triangle writes its index into its tiles'
//     bins (slot order depends on scheduling, the minimum does not);
//   * tiles (one workgroup per tile, 256 lanes x 4 adjacent pixels of one row): load the current depth, walk the tile's bin and the
//     large list 256 entries at a time -- the lanes first drop the records that cannot touch the tile (box, and an edge function
//     negative over the whole tile), the rest go through LDS --, evaluate the exact int64 edge functions at the pixel centres with the
//     top-left rule, interpolate z in fp64, keep the minimum in registers and store once.  No atomics touch the depth map.
// Scratch sizes follow from the triangle count and the target size alone (pbrk_raster_scratch_bytes): no read-back.
// What K13 needs as well lives in raster_bins.h: record, pixel box, draw lookup, counting, scan, fill, pre-filter, the batch loop of
// the tile kernel and the launch sequence of setup.  This file keeps the transform and guard band of setup and the depth minimum of
// the tile body.
#include "pbr_kernels.h"
#include "raster_bins.h"

#include <hip/hip_runtime.h>

#include <float.h>
#include <math.h>

namespace {

__global__ __launch_bounds__(kThreads) void k_raster_setup(PbrkRasterArgs a, Layout L) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    bool rejected = false;
    unsigned key = kNoKey;                                          // the one tile of a single-tile triangle
    char* scratch = (char*)a.scratch;
    if (t < a.tri_count) {
        const PbrkRasterDraw* d = &a.draws[find_draw(a.draws, a.draw_count, t)];
        const uint32_t* ix = a.indices + (size_t)d->first_index + 3 * (size_t)(t - d->first_tri);   // in range: checked at record time
        const float hw = (float)a.width * 0.5f, hh = (float)a.height * 0.5f;
        int X[3] = {0, 0, 0}, Y[3] = {0, 0, 0};
        float Z[3] = {0.0f, 0.0f, 0.0f};
        bool ok = true;
        for (int k = 0; k < 3 && ok; ++k) {
            const unsigned long long v = (unsigned long long)ix[k] + d->vertex_offset;
            if (v >= a.vertex_count) { ok = false; break; }
            const float* p = (const float*)((const char*)a.vertices + v * a.vertex_stride);
            const float x = p[0], y = p[1], z = p[2];
            const float cx = ((d->m[0] * x + d->m[4] * y) + d->m[8] * z) + d->m[12];
            const float cy = ((d->m[1] * x + d->m[5] * y) + d->m[9] * z) + d->m[13];
            const float cz = ((d->m[2] * x + d->m[6] * y) + d->m[10] * z) + d->m[14];
            const float cw = ((d->m[3] * x + d->m[7] * y) + d->m[11] * z) + d->m[15];
            const float xd = cx / cw, yd = cy / cw, zd = cz / cw;
            const float xf = hw * xd + hw, yf = hh * yd + hh;
            if (!(fabsf(xf) <= 2097152.0f) || !(fabsf(yf) <= 2097152.0f) || !(fabsf(zd) <= FLT_MAX)) { ok = false; break; }
            X[k] = (int)rintf(xf * 256.0f); Y[k] = (int)rintf(yf * 256.0f); Z[k] = zd;
        }
        rejected = !ok;
        TriRec r;
        r.x0 = X[0]; r.y0 = Y[0]; r.x1 = X[1]; r.y1 = Y[1]; r.x2 = X[2]; r.y2 = Y[2];
        r.z0 = Z[0];
        const long long area = ((long long)X[1] - X[0]) * ((long long)Y[2] - Y[0]) - ((long long)Y[1] - Y[0]) * ((long long)X[2] - X[0]);
        if (ok && area != 0) {
            r.set_box(pixel_box(X[0], Y[0], X[1], Y[1], X[2], Y[2], a.width, a.height));
            if (!r.box().empty()) {
                r.inv = 1.0 / (double)area;
                r.dz1 = (double)Z[1] - (double)Z[0];
                r.dz2 = (double)Z[2] - (double)Z[0];
            }
        }
        store_rec(scratch, L, t, r);
        if (!r.box().empty()) key = count_box(scratch, L, r.box(), t, true);
    }
    const unsigned long long m = __ballot(rejected);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.rejected, (unsigned long long)__popcll(m));
    wave_take((unsigned*)(scratch + L.cnt), key);                   // the single-tile triangles of the wave
}

__global__ __launch_bounds__(kThreads) void k_raster_tiles(PbrkRasterArgs a, Layout L) {
    __shared__ int4 lds[kThreads * 4];                                      // 256 records, 16 KB
    __shared__ unsigned kept[kThreads];
    __shared__ unsigned nkept;
    const int py = blockIdx.y * kTile + (threadIdx.x >> 3);                 // this lane: the four pixels (px .. px + 3, py)
    const int px = blockIdx.x * kTile + (threadIdx.x & 7) * 4;
    const int W = a.width, H = a.height;
    const bool row_in = py < H;
    const bool vec = row_in && (W & 3) == 0 && px + 3 < W;
    float cur[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    float* row = a.depth + (size_t)(row_in ? py : 0) * W;
    if (vec) {
        const float4 v = *(const float4*)(row + px);
        cur[0] = v.x; cur[1] = v.y; cur[2] = v.z; cur[3] = v.w;
    } else if (row_in) {
        for (int q = 0; q < 4; ++q) if (px + q < W) cur[q] = row[px + q];
    }
    const TriRec* sr = (const TriRec*)lds;
    walk_tile((const char*)a.scratch, L, lds, kept, &nkept, [&](unsigned k) {
        const TriRec& r = sr[k];
        const PixBox b = r.box();
        if (py < b.y0 || py > b.y1 || px + 3 < b.x0 || px > b.x1) return;
        const long long x0 = r.x0, y0 = r.y0, x1 = r.x1, y1 = r.y1, x2 = r.x2, y2 = r.y2;
        const bool pos = r.inv > 0.0;                                       // orientation: both windings are drawn
        // E0 = edge(v1 -> v2), E1 = edge(v2 -> v0), E2 = edge(v0 -> v1); edge(a -> b, p) = (b.x - a.x)(p.y - a.y) - (b.y - a.y)(p.x - a.x)
        const long long Px = 256LL * px + 128, Py = 256LL * py + 128;
        long long e0 = (x2 - x1) * (Py - y1) - (y2 - y1) * (Px - x1);
        long long e1 = (x0 - x2) * (Py - y2) - (y0 - y2) * (Px - x2);
        long long e2 = (x1 - x0) * (Py - y0) - (y1 - y0) * (Px - x0);
        const long long d0 = -(y2 - y1) * 256, d1 = -(y0 - y2) * 256, d2 = -(y1 - y0) * 256;
        // top-left rule (y down): with the edge functions oriented positive inside, a centre ON an edge is covered when the
        // inward normal (A, B) has A > 0 (left edge) or A == 0 and B > 0 (top edge)
        const long long sg = pos ? 1 : -1;
        const long long b0 = top_left(-(y2 - y1) * sg, (x2 - x1) * sg) ? 0 : 1;
        const long long b1 = top_left(-(y0 - y2) * sg, (x0 - x2) * sg) ? 0 : 1;
        const long long b2 = top_left(-(y1 - y0) * sg, (x1 - x0) * sg) ? 0 : 1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long n0 = pos ? e0 : -e0, n1 = pos ? e1 : -e1, n2 = pos ? e2 : -e2;
            const int x = px + q;
            if (n0 >= b0 && n1 >= b1 && n2 >= b2 && x >= b.x0 && x <= b.x1) {
                const double z = (double)r.z0 + ((double)e1 * r.dz1 + (double)e2 * r.dz2) * r.inv;
                float zf = (float)z;
                if (zf >= 0.0f && zf <= 1.0f) {
                    if (zf == 0.0f) zf = 0.0f;                              // -0 -> +0
                    if (zf < cur[q]) cur[q] = zf;                           // LESS
                }
            }
            e0 += d0; e1 += d1; e2 += d2;
        }
    });
    if (vec) {
        *(float4*)(row + px) = make_float4(cur[0], cur[1], cur[2], cur[3]);
    } else if (row_in) {
        for (int q = 0; q < 4; ++q) if (px + q < W) row[px + q] = cur[q];
    }
}

bool args_ok(const PbrkRasterArgs* a) {
    return a && a->vertices && a->indices && a->draws && a->depth && a->scratch && a->rejected && a->draw_count > 0 &&
           dims_ok(a->width, a->height) && a->vertex_stride >= 12 && (a->vertex_stride & 3) == 0;
}
}  // namespace

extern "C" size_t pbrk_raster_scratch_bytes(uint32_t tri_count, int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    return raster_layout(tri_count, width, height).total;
}

extern "C" int pbrk_raster_setup(const PbrkRasterArgs* a, void* stream) {
    if (!args_ok(a)) return PBRK_E_ARG;
    if (a->tri_count == 0) return PBRK_OK;
    const Layout L = raster_layout(a->tri_count, a->width, a->height);
    return launch_binning(k_raster_setup, *a, L, a->tri_count, (hipStream_t)stream) ? PBRK_OK : PBRK_E_LAUNCH;
}

extern "C" int pbrk_raster_tiles(const PbrkRasterArgs* a, void* stream) {
    if (!args_ok(a)) return PBRK_E_ARG;
    if (a->tri_count == 0) return PBRK_OK;
    const Layout L = raster_layout(a->tri_count, a->width, a->height);
    hipLaunchKernelGGL(k_raster_tiles, dim3(L.tx, L.ty), dim3(kThreads), 0, (hipStream_t)stream, *a, L);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}
