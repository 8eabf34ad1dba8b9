// raster_bins.h -- the raster-job machinery of the compute rasterisers K12 (k_raster.hip) and K13 (k_geometry.hip): the 64-B coverage
// record and its pixel box, the scratch layout, the draw lookup, counting into tiles (count_box), the scan and fill kernels that turn
// the counts into bins, the per-tile pre-filter (meets_tile), the batch loop of the tile kernels (walk_list) and the launch sequence
// of a setup (launch_binning).  A pass adds its setup kernel and the per-record body of its tile kernel.  Each translation unit that
// includes it gets its own copy of the two kernels (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
constexpr int kTile = 32;                 // tile edge in pixels
constexpr int kMaxTiles = 16;             // a record whose pixel box touches more tiles goes to the large list
constexpr int kThreads = 256;
constexpr unsigned kNoKey = 0xFFFFFFFFu;  // "no tile"

struct PixBox {                           // inclusive pixel range; x0 > x1 or y0 > y1: empty
    int x0, y0, x1, y1;
    __host__ __device__ bool empty() const { return x0 > x1 || y0 > y1; }
};

struct alignas(16) TriRec {               // 64 B, all zero but for an empty box until a setup kernel fills it
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0, x2 = 0, y2 = 0;     // snapped framebuffer coordinates, 1/256 px
    short bx0 = 1, by0 = 1, bx1 = 0, by1 = 0;               // pixel box, clamped to the target: within [0, 16383], or (1, 1) .. (0, 0)
    float z0 = 0.0f, pad = 0.0f;          // K13 keeps the source triangle's number in `pad` (bit pattern)
    double inv = 0.0, dz1 = 0.0, dz2 = 0.0;                 // 1 / (E0 + E1 + E2), z1 - z0, z2 - z0
    __device__ PixBox box() const { return PixBox{bx0, by0, bx1, by1}; }
    __device__ void set_box(const PixBox& b) { bx0 = (short)b.x0; by0 = (short)b.y0; bx1 = (short)b.x1; by1 = (short)b.y1; }
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

inline bool dims_ok(int width, int height) { return width > 0 && height > 0 && width <= 16384 && height <= 16384; }

__device__ inline bool top_left(long long a, long long b) { return a > 0 || (a == 0 && b > 0); }

// the last draw with first_tri <= t (first_tri ascending, draws[0].first_tri == 0)
template <class Draw>
__device__ inline int find_draw(const Draw* draws, uint32_t draw_count, uint32_t t) {
    int lo = 0, hi = (int)draw_count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (draws[mid].first_tri <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the pixels whose centres 256 i + 128 lie inside the bounding box of three snapped vertices, clamped to the W x H target; (1, 1) ..
// (0, 0) when there is none
__device__ inline PixBox pixel_box(long long x0, long long y0, long long x1, long long y1, long long x2, long long y2, int W, int H) {
    const long long mnx = x0 < x1 ? (x0 < x2 ? x0 : x2) : (x1 < x2 ? x1 : x2);
    const long long mxx = x0 > x1 ? (x0 > x2 ? x0 : x2) : (x1 > x2 ? x1 : x2);
    const long long mny = y0 < y1 ? (y0 < y2 ? y0 : y2) : (y1 < y2 ? y1 : y2);
    const long long mxy = y0 > y1 ? (y0 > y2 ? y0 : y2) : (y1 > y2 ? y1 : y2);
    long long i0 = (mnx + 127) >> 8, i1 = (mxx - 128) >> 8, j0 = (mny + 127) >> 8, j1 = (mxy - 128) >> 8;
    if (i0 < 0) i0 = 0;
    if (j0 < 0) j0 = 0;
    if (i1 > W - 1) i1 = W - 1;
    if (j1 > H - 1) j1 = H - 1;
    if (i0 > i1 || j0 > j1) return PixBox{1, 1, 0, 0};
    return PixBox{(int)i0, (int)j0, (int)i1, (int)j1};
}

__device__ inline void store_rec(char* scratch, const Layout& L, size_t slot, const TriRec& r) {
    const int4* src = (const int4*)&r;
    int4* dst = (int4*)(scratch + L.rec) + 4 * slot;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
}

// the one tile a non-empty box lies in, or kNoKey
__device__ inline unsigned single_tile(const PixBox& b, int tiles_x) {
    const int tx0 = b.x0 >> 5, ty0 = b.y0 >> 5;
    return tx0 == (b.x1 >> 5) && ty0 == (b.y1 >> 5) ? (unsigned)(ty0 * tiles_x + tx0) : kNoKey;
}

// f(tile) for every tile a non-empty box is binned into; false, and no call, when it touches more than kMaxTiles (the large list)
template <class F>
__device__ inline bool each_tile(const PixBox& b, int tiles_x, F f) {
    const int tx0 = b.x0 >> 5, tx1 = b.x1 >> 5, ty0 = b.y0 >> 5, ty1 = b.y1 >> 5;
    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > kMaxTiles) return false;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) f(ty * tiles_x + tx);
    return true;
}

// One atomic per distinct key of the wave (consecutive triangles of a part mostly fall into the same tile): adds to counters[key] the
// number of lanes that hold `key` and returns this lane's slot among them.  Every lane of the wave calls it; kNoKey takes nothing.
__device__ inline unsigned wave_take(unsigned* counters, unsigned key) {
    const int lane = threadIdx.x & 63;
    unsigned slot = 0;
    unsigned long long todo = __ballot(key != kNoKey);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned k = __shfl(key, leader);
        const unsigned long long grp = __ballot(key == k);
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(&counters[k], (unsigned)__popcll(grp));
        base = __shfl(base, leader);
        if (key == k) slot = base + (unsigned)__popcll(grp & ((1ull << lane) - 1ull));
        todo &= ~grp;
    }
    return slot;
}

// Setup: count record `rec` with the non-empty box `b` into the tiles it touches, or append it to the large list.  With `aggregate`,
// a box inside one tile is not counted here: its tile is returned, for the caller's wave_take on the counts.
__device__ inline unsigned count_box(char* scratch, const Layout& L, const PixBox& b, unsigned rec, bool aggregate) {
    unsigned* cnt = (unsigned*)(scratch + L.cnt);
    const unsigned key = aggregate ? single_tile(b, L.tx) : kNoKey;
    if (key != kNoKey) return key;
    if (!each_tile(b, L.tx, [&](int tile) { atomicAdd(&cnt[tile], 1u); })) {
        const unsigned slot = atomicAdd(&cnt[L.ntiles], 1u);                  // < number of records
        ((unsigned*)(scratch + L.large))[slot] = rec;
    }
    return kNoKey;
}

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

// every binned record writes its index into its tiles' bins: the tiles of each_tile, slots inside the range the counts gave the tile
__global__ __launch_bounds__(kThreads) void k_raster_fill(char* scratch, uint32_t n, Layout L) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    unsigned* cur = (unsigned*)(scratch + L.cur);
    unsigned* bins = (unsigned*)(scratch + L.bins);
    unsigned key = kNoKey;
    if (t < n) {
        const PixBox b = ((const TriRec*)(scratch + L.rec))[t].box();
        if (!b.empty()) {
            key = single_tile(b, L.tx);
            if (key == kNoKey) each_tile(b, L.tx, [&](int tile) { bins[atomicAdd(&cur[tile], 1u)] = t; });
        }
    }
    const unsigned slot = wave_take(cur, key);                              // single-tile records, whichever way the setup counted them
    if (key != kNoKey) bins[slot] = t;
}

// Can a record cover a pixel centre of the tile [px0, px0 + 31] x [py0, py0 + 31]?  Its pixel box must meet the tile, and no edge
// function may be negative at every centre of it (an affine function's maximum over the tile is at the corner its gradient points to).
__device__ inline bool meets_tile(const TriRec& r, int px0, int py0) {
    const PixBox b = r.box();
    if (b.empty() || b.x1 < px0 || b.x0 > px0 + kTile - 1 || b.y1 < py0 || b.y0 > py0 + kTile - 1) return false;
    const long long x0 = r.x0, y0 = r.y0, x1 = r.x1, y1 = r.y1, x2 = r.x2, y2 = r.y2;
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

// One list (a tile's bin or the large list) of a tile kernel, 256 entries at a time: the lanes first keep the entries that can touch
// the tile at (tx0, ty0) (meets_tile), the kept records are staged in `lds` (256 TriRec), then every lane calls body(k) for each
// staged record k.  The order of the records depends on scheduling; what a body computes must not.
template <class Body>
__device__ __forceinline__ void walk_list(const unsigned* list, unsigned n, const TriRec* recs, int4* lds, unsigned* kept, unsigned* nkept,
                                          int tx0, int ty0, Body body) {
    for (unsigned base = 0; base < n; base += kThreads) {
        __syncthreads();                                                    // the previous batch is consumed
        if (threadIdx.x == 0) *nkept = 0;
        __syncthreads();
        const unsigned j = base + threadIdx.x;
        if (j < n) {
            const unsigned t = list[j];
            if (meets_tile(recs[t], tx0, ty0)) kept[atomicAdd(nkept, 1u)] = t;                  // LDS counter
        }
        __syncthreads();
        const unsigned m = *nkept;
        if (threadIdx.x < m) {
            const int4* src = (const int4*)(recs + kept[threadIdx.x]);
            int4* d = lds + 4 * threadIdx.x;
            d[0] = src[0]; d[1] = src[1]; d[2] = src[2]; d[3] = src[3];
        }
        __syncthreads();
        for (unsigned k = 0; k < m; ++k) body(k);
    }
}

// what a tile kernel's workgroup walks: its tile's bin, then the large list
template <class Body>
__device__ __forceinline__ void walk_tile(const char* scratch, const Layout& L, int4* lds, unsigned* kept, unsigned* nkept, Body body) {
    const unsigned* cnt = (const unsigned*)(scratch + L.cnt);
    const unsigned* off = (const unsigned*)(scratch + L.off);
    const TriRec* recs = (const TriRec*)(scratch + L.rec);
    const int tile = blockIdx.y * L.tx + blockIdx.x, tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
    walk_list((const unsigned*)(scratch + L.bins) + off[tile], off[tile + 1] - off[tile], recs, lds, kept, nkept, tx0, ty0, body);
    walk_list((const unsigned*)(scratch + L.large), cnt[L.ntiles], recs, lds, kept, nkept, tx0, ty0, body);
}

// A setup launch: clear the counts, `setup` (one thread per triangle, writes and counts `nrec` records), scan, fill.
template <class Args>
inline bool launch_binning(void (*setup)(Args, Layout), const Args& a, const Layout& L, uint32_t nrec, hipStream_t st) {
    if (hipMemsetAsync((char*)a.scratch + L.cnt, 0, ((size_t)L.ntiles + 1) * 4, st) != hipSuccess) return false;
    hipLaunchKernelGGL(setup, dim3((a.tri_count + kThreads - 1) / kThreads), dim3(kThreads), 0, st, a, L);
    hipLaunchKernelGGL(k_raster_scan, dim3(1), dim3(1024), 0, st, (char*)a.scratch, L);
    hipLaunchKernelGGL(k_raster_fill, dim3((nrec + kThreads - 1) / kThreads), dim3(kThreads), 0, st, (char*)a.scratch, nrec, L);
    return hipGetLastError() == hipSuccess;
}
}  // namespace
