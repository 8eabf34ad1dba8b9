// raster_bins.h -- what the compute rasterisers K12 (k_raster.hip) and K13 (k_geometry.hip) share: the 64-B coverage record, the
// scratch layout, the scan and fill kernels that turn per-tile counts into bins, and the per-tile pre-filter.  Each translation
// unit that includes it gets its own copy of the two kernels (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
constexpr int kTile = 32;                 // tile edge in pixels
constexpr int kMaxTiles = 16;             // a record whose pixel box touches more tiles goes to the large list
constexpr int kThreads = 256;

struct TriRec {                           // 64 B; bx0 > bx1 marks a record that covers nothing
    int x0, y0, x1, y1, x2, y2;           // snapped framebuffer coordinates, 1/256 px
    short bx0, by0, bx1, by1;             // pixel box, clamped to the target
    float z0, pad;                        // K13 keeps the source triangle's number in `pad` (bit pattern)
    double inv, dz1, dz2;                 // 1 / (E0 + E1 + E2), z1 - z0, z2 - z0
};
static_assert(sizeof(TriRec) == 64, "TriRec is four 16-B words");

struct Layout {
    size_t rec, cnt, off, cur, bins, large, extra, total;
    int tx, ty, ntiles;
};

// n records; `extra_bytes` more for the caller's own per-triangle data (K13's attribute records)
inline Layout raster_layout(uint32_t n, int W, int H, size_t extra_bytes = 0) {
    Layout L;
    L.tx = (W + kTile - 1) / kTile; L.ty = (H + kTile - 1) / kTile; L.ntiles = L.tx * L.ty;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    L.rec = take((size_t)n * sizeof(TriRec));
    L.cnt = take(((size_t)L.ntiles + 1) * 4);           // per-tile counts, then the large-list count
    L.off = take(((size_t)L.ntiles + 1) * 4);           // exclusive prefix of the counts
    L.cur = take((size_t)L.ntiles * 4);                 // fill cursors
    L.bins = take((size_t)kMaxTiles * n * 4);
    L.large = take((size_t)n * 4);
    L.extra = take(extra_bytes);
    L.total = o > 256 ? o : 256;
    return L;
}

__device__ inline bool top_left(long long a, long long b) { return a > 0 || (a == 0 && b > 0); }

// exclusive prefix of the tile counts: 1024 threads, each a contiguous chunk
__global__ __launch_bounds__(1024) void k_raster_scan(char* scratch, Layout L) {
    __shared__ unsigned part[1024];
    const unsigned* cnt = (const unsigned*)(scratch + L.cnt);
    unsigned* off = (unsigned*)(scratch + L.off);
    unsigned* cur = (unsigned*)(scratch + L.cur);
    const int n = L.ntiles, chunk = (n + 1023) / 1024;
    const int b = threadIdx.x * chunk, e = b + chunk < n ? b + chunk : n;
    unsigned s = 0;
    for (int i = b; i < e; ++i) s += cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                                  // inclusive Hillis-Steele
        const unsigned v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned run = part[threadIdx.x] - s;
    for (int i = b; i < e; ++i) { off[i] = run; cur[i] = run; run += cnt[i]; }
    if (threadIdx.x == 1023) off[n] = part[1023];
}

__global__ __launch_bounds__(kThreads) void k_raster_fill(char* scratch, uint32_t n, Layout L) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    unsigned* cur = (unsigned*)(scratch + L.cur);
    unsigned* bins = (unsigned*)(scratch + L.bins);
    unsigned key = 0xFFFFFFFFu;
    if (t < n) {
        const TriRec* r = (const TriRec*)(scratch + L.rec) + t;
        const int bx0 = r->bx0, bx1 = r->bx1, by0 = r->by0, by1 = r->by1;
        if (bx0 <= bx1 && by0 <= by1) {
            const int tx0 = bx0 >> 5, tx1 = bx1 >> 5, ty0 = by0 >> 5, ty1 = by1 >> 5;
            if (tx0 == tx1 && ty0 == ty1) {
                key = (unsigned)(ty0 * L.tx + tx0);
            } else if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) <= kMaxTiles) {
                for (int ty = ty0; ty <= ty1; ++ty)
                    for (int tx = tx0; tx <= tx1; ++tx) bins[atomicAdd(&cur[ty * L.tx + tx], 1u)] = t;   // slots stay inside the tile's range
            }
        }
    }
    // single-tile records: the wave's lanes of one tile take consecutive slots from one atomic (the counts of the setup match)
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(key != 0xFFFFFFFFu);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned k = __shfl(key, leader);
        const unsigned long long grp = __ballot(key == k);
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(&cur[k], (unsigned)__popcll(grp));
        base = __shfl(base, leader);
        if (key == k) bins[base + (unsigned)__popcll(grp & ((1ull << lane) - 1ull))] = t;
        todo &= ~grp;
    }
}

// Can a record cover a pixel centre of the tile [px0, px0 + 31] x [py0, py0 + 31]?  Its pixel box must meet the tile, and no edge
// function may be negative at every centre of it (an affine function's maximum over the tile is at the corner its gradient points to).
__device__ inline bool meets_tile(const int4* rec, int px0, int py0) {
    const int4 w0 = rec[0], w1 = rec[1];                                    // x0 y0 x1 y1 | x2 y2 (bx0, by0) (bx1, by1)
    const int bx0 = (short)(w1.z & 0xFFFF), by0 = w1.z >> 16, bx1 = (short)(w1.w & 0xFFFF), by1 = w1.w >> 16;
    if (bx0 > bx1 || by0 > by1 || bx1 < px0 || bx0 > px0 + kTile - 1 || by1 < py0 || by0 > py0 + kTile - 1) return false;
    const long long x0 = w0.x, y0 = w0.y, x1 = w0.z, y1 = w0.w, x2 = w1.x, y2 = w1.y;
    const long long sg = ((x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)) > 0 ? 1 : -1;
    const long long lo_x = 256LL * px0 + 128, hi_x = lo_x + 256LL * (kTile - 1), lo_y = 256LL * py0 + 128, hi_y = lo_y + 256LL * (kTile - 1);
    const long long ex[3][4] = {{x1, y1, x2, y2}, {x2, y2, x0, y0}, {x0, y0, x1, y1}};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long ax = ex[k][0], ay = ex[k][1], bxx = ex[k][2], byy = ex[k][3];
        const long long A = -(byy - ay) * sg, B = (bxx - ax) * sg;           // oriented gradient
        const long long Px = A > 0 ? hi_x : lo_x, Py = B > 0 ? hi_y : lo_y;
        if (sg * ((bxx - ax) * (Py - ay) - (byy - ay) * (Px - ax)) < 0) return false;
    }
    return true;
}
}  // namespace
