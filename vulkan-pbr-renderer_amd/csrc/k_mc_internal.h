// k_mc_internal.h -- argument block shared by the Monte-Carlo filter kernels (k_mc.hip, k_mc_region.hip, k_mc_prep.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include "pbr_device.h"
#include "mc_plan.h"

struct McArgs {
    const float4* src; int n_src; unsigned src_bytes;
    const float4* cells; unsigned cells_bytes;          // optional 2x2-footprint layout: 3 loads per sample instead of 4
    const float4* tab; int n_tab;
    float divisor, alpha;
    float4* out; int size;
    int face0, y0, rows, tiles_x, tiles_per_face;
    int snap;                                           // host side: cube-sampler convention (pbrk_set_cube_sampler_snap) -> the SNAP instantiation of the direct kernel
};

typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));


__device__ __forceinline__ f3 tap_rgb(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
    u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(rs, voff, soff, 0);
    return mk3(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z));
}

// "cells" layout (pbr_device.h, cells_bilerp): for every tap position (face, j0, i0), i0/j0 in [0, n], the 2x2 RGB footprint in
// coefficient form {t00, t10 - t00, t01, t11 - t01}, 48 contiguous bytes -> three 16-byte loads and 12 instructions per fetch.
typedef unsigned int u32x4c __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f3 fetch_cells(__amdgpu_buffer_rsrc_t rc, int voff, float a, float b) {
    u32x4c A = __builtin_amdgcn_raw_buffer_load_b128(rc, voff, 0, 0);
    u32x4c Bq = __builtin_amdgcn_raw_buffer_load_b128(rc, voff + 16, 0, 0);
    u32x4c Cq = __builtin_amdgcn_raw_buffer_load_b128(rc, voff + 32, 0, 0);
    return cells_bilerp(make_float4(__uint_as_float(A.x), __uint_as_float(A.y), __uint_as_float(A.z), __uint_as_float(A.w)),
                        make_float4(__uint_as_float(Bq.x), __uint_as_float(Bq.y), __uint_as_float(Bq.z), __uint_as_float(Bq.w)),
                        make_float4(__uint_as_float(Cq.x), __uint_as_float(Cq.y), __uint_as_float(Cq.z), __uint_as_float(Cq.w)), a, b);
}

// one sample: direction L -> bilinear RGB of the bordered level behind `rs`
template <bool CELLS>
__device__ __forceinline__ f3 sample_bordered(__amdgpu_buffer_rsrc_t rs, f3 L, float nf, float off, int nb, int row_bytes, bool snap = false) {
    float fid = __builtin_amdgcn_cubeid(L.x, L.y, L.z);
    float sc = __builtin_amdgcn_cubesc(L.x, L.y, L.z);
    float tc = __builtin_amdgcn_cubetc(L.x, L.y, L.z);
    float ma2 = __builtin_amdgcn_cubema(L.x, L.y, L.z);          // 2 * major axis
    float h = __builtin_amdgcn_rcpf(fabsf(ma2)) * nf;            // n / (2 |rc|)
    float u = fmaf(sc, h, off);                                  // s*n - 0.5 + 1 (bordered), in [0.5, n + 0.5]
    float v = fmaf(tc, h, off);
    if (snap) { u = snap256(u); v = snap256(v); }                // bordered = unbordered + 1: the snap commutes with the offset
    float a = __builtin_amdgcn_fractf(u), b = __builtin_amdgcn_fractf(v);
    if (CELLS) {
        // Cell byte offset in fp32: cells exist for n <= 512 only, so face*nc + j0, the cell index (< 6*513^2 < 2^24) and
        // 48*cell (= 16 * an integer < 2^24) are all exact -- six FMA-rate instructions instead of three conversions and three
        // integer multiplies (v_mul_lo_u32 / v_mad_u64_u32 issue at 1.45x / 1.7x the cost of an FMA here, tools/ubench_valu.hip).
        float ncf = (float)(nb - 1);                             // n + 1 tap positions per edge
        float cellf = fmaf(fmaf(fid, ncf, floorf(v)), ncf, floorf(u));
        return fetch_cells(rs, (int)(cellf * (float)PBR_CELL_BYTES), a, b);
    }
    int i0 = (int)u, j0 = (int)v, face = (int)fid;
    int voff = ((face * nb + j0) * nb + i0) << 4;
    f3 t00 = tap_rgb(rs, voff, 0), t10 = tap_rgb(rs, voff + 16, 0);
    f3 t01 = tap_rgb(rs, voff, row_bytes), t11 = tap_rgb(rs, voff + 16, row_bytes);
    f3 r;
    r.x = lerp_fma(lerp_fma(t00.x, t10.x, a), lerp_fma(t01.x, t11.x, a), b);
    r.y = lerp_fma(lerp_fma(t00.y, t10.y, a), lerp_fma(t01.y, t11.y, a), b);
    r.z = lerp_fma(lerp_fma(t00.z, t10.z, a), lerp_fma(t01.z, t11.z, a), b);
    return r;
}

// k_mc_region.hip: the k-th region a tile visits -- the GG regions of its own face (first region: own) first, then all the
// others in index order.  A permutation of 0 .. NR-1 that depends on the face only.
__host__ __device__ __forceinline__ int mc_region_visit(int k, int own, int GG) {
    return k < GG ? own + k : (k < own + GG ? k - GG : k);
}

// k_mc_region.hip, header 2g: the launch-level cut.  Slice s of the sample table owns the mask words s, s + 4, ..; word s is its head,
// run first over every region (head phase), the others are its tail.  wbits[NW]: per mask word the largest bit pattern of its
// samples' weights (W_w); H[s]: the sum of the 32 weights of head word s, added in index order in double; min_bits / max_bits: the
// smallest / largest R, G, B bit pattern of the bordered source level (m, M).  Tail word w of slice s is cut when every word
// w' >= w of the slice satisfies, in double and evaluated left to right,
//     W_w' * M * 2^25 * (1 + 2^-10) <= H_s * m
// with m a normal positive float, M finite, every weight >= +0 (a bit pattern below +inf's) and H_s m 2^-25 >= 2^-100.  Then every
// lane's three sums are at least H_s m (1 - 2^-12) once the head phase is over (each head sample is taken exactly once, its tap
// weights are monotone roundings that add up to its weight within a few ulp, every tap is >= m, and 128 FMAs lose under 2^-17
// relative), they never fall afterwards (all products >= 0), and every product of a cut word is <= W M <= acc 2^-25: by the
// lemma at absorb_threshold each of its FMAs returns its sum unchanged, for every lane of every tile.  cut4[s]: the first cut
// word of slice s, or the first index of the slice at or behind NW when none is cut.  Returns the number of words cut; 0 for tables
// of at most 128 samples (one phase, no tail).
// mc_launch_cut_s: the same for a launch whose workgroups own S slices (S = 1024 / TILE^2: 4 with 16 x 16 tiles, 1 with 32 x 32; header
// 2h): slice s owns the words s, s + S, .., its head is word s, H has S entries and cut[s], s < S, is written.  No tail, no cut: NW <= S.
__host__ __device__ inline int mc_launch_cut_s(const unsigned* wbits, int NW, int S, const double* H, unsigned min_bits, unsigned max_bits, int* cut) {
    for (int s = 0; s < S; ++s) cut[s] = s >= NW ? s : s + S * ((NW - s + S - 1) / S);
    if (NW <= S) return 0;
    if (min_bits < 0x00800000u || min_bits >= 0x7f800000u || max_bits >= 0x7f800000u) return 0;
    for (int w = 0; w < NW; ++w)
        if (wbits[w] >= 0x7f800000u) return 0;
    union { unsigned u; float f; } cm, cM, cW;
    cm.u = min_bits; cM.u = max_bits;
    const double m = (double)cm.f, M = (double)cM.f;
    int ncut = 0;
    for (int s = 0; s < S; ++s) {
        const double rhs = H[s] * m;
        if (!(rhs * 0x1p-25 >= 0x1p-100)) continue;                // NaN fails
        int c = cut[s];
        for (int w = c - S; w > s; w -= S) {
            cW.u = wbits[w];
            const double lhs = (double)cW.f * M * 0x1p25 * (1.0 + 0x1p-10);
            if (!(lhs <= rhs)) break;
            c = w;
        }
        ncut += (cut[s] - c) / S;
        cut[s] = c;
    }
    return ncut;
}
__host__ __device__ inline int mc_launch_cut(const unsigned* wbits, int NW, const double* H, unsigned min_bits, unsigned max_bits, int* cut4) {
    return mc_launch_cut_s(wbits, NW, 4, H, min_bits, max_bits, cut4);
}

// k_mc_region.hip, header 2l: mono[s], s < S, is the first word of slice s (words s, s + S, .. below NW) from which the slice's word maxima
// wbits[] never rise again -- compared as bit patterns, which for weights >= +0 is their order as floats; a slice without words gets s.
// A pass of the net-less kernel that finds a word w >= mono[s] absorbed ends there: every later word of the slice has a maximum, hence a
// threshold (absorb_threshold is monotone in the word maximum for one region maximum), no larger, and the sums have not moved.
__host__ __device__ inline void mc_mono_from(const unsigned* wbits, int NW, int S, int* mono) {
    for (int s = 0; s < S; ++s) {
        int k = s;
        if (s < NW) {
            k = s + S * ((NW - 1 - s) / S);                            // the slice's last word: monotone on its own
            while (k - S >= s && wbits[k - S] >= wbits[k]) k -= S;
        }
        mono[s] = k;
    }
}

// k_mc_region.hip, tile_of_block: block -> (face, tx, ty) of a dispatch of tiles_per_face = tiles_x * tiles_y tiles per face that starts
// at face0; ty counts from the dispatch's first tile row.  Tiles in plain block order but for the faces +X / -X, whose rows are dealt
// outwards from pole_row[face] (the comment at tile_of_block says why).  A bijection of the dispatch's blocks onto its tiles.
__host__ __device__ __forceinline__ void mc_tile_of_block(unsigned block, int face0, int tiles_x, int tiles_per_face, const int* pole_row,
                                                          int& face, int& tx, int& ty) {
    face = face0 + (int)(block / (unsigned)tiles_per_face);
    const int tf = (int)(block % (unsigned)tiles_per_face);
    ty = tf / tiles_x;
    tx = tf % tiles_x;
    if (face < 2) {
        const int ny = tiles_per_face / tiles_x, pr = pole_row[face];
        const int a = pr < ny - 1 - pr ? pr : ny - 1 - pr;
        if (ty <= 2 * a) { const int h = (ty + 1) >> 1; ty = (ty & 1) ? pr + h : pr - h; }
        else { const int rest = ty - 2 * a; ty = (pr > ny - 1 - pr) ? pr - a - rest : pr + a + rest; }
    }
}

// Tile row (relative to the tiles' first row y0, clamped) of the tangent frame's pole on faces +X (t = (1 - vy/vx)/2) and -X
// (t = (1 + vy/vx)/2), v = the vector of tangent_of: mc_tile_of_block deals the rows of these faces outwards from it
inline void mc_pole_rows(int size, int y0, int tile, int tiles_y, int* pole_row) {
    const double vy_vx = 6.11831989512 / 12.123825810901;
    for (int f = 0; f < 2; ++f) {
        int row = (int)((f == 0 ? 0.5 * (1.0 - vy_vx) : 0.5 * (1.0 + vy_vx)) * size);
        int tr = (row - y0) / tile;
        if (row < y0) tr = 0;
        pole_row[f] = tr < 0 ? 0 : (tr > tiles_y - 1 ? tiles_y - 1 : tr);
    }
}

// k_mc_region.hip, header 2m: the bin cache.  A tile's flags are masks[NR][NW], then cmask[NW]; tiles lie [face][tile row from row 0 of
// the face][tile column], each on a stride of whole 16-byte groups so that a lane's 16-byte load never straddles two tiles.
__host__ __device__ __forceinline__ unsigned mc_bin_tile_words(int NR, int NW) { return ((unsigned)(NR + 1) * (unsigned)NW + 3u) & ~3u; }
// the index of tile (face, first_row + ty, tx): first_row = the dispatch's first tile row, counted from row 0 of the face
__host__ __device__ __forceinline__ unsigned mc_bin_tile_index(int face, int first_row, int ty, int tx, int tiles_x, int tiles_y_face) {
    return (unsigned)((face * tiles_y_face + first_row + ty) * tiles_x + tx);
}
// Which row windows [y0, y1) of the region kernel may use the cache: its tiles start at the dispatch's first row and their frames clamp at
// its last, so the window must start on a tile row of the whole-face dispatch and end on one or at the face's end.
__host__ __device__ __forceinline__ bool mc_bin_window_ok(int size, int tile, int y0, int y1) {
    return y0 >= 0 && y0 < y1 && y1 <= size && y0 % tile == 0 && (y1 % tile == 0 || y1 == size);
}

// k_mc_region.hip: taps from LDS-staged regions of the source level.  Returns false when the kernel does not apply
// (the caller then takes the direct kernel); the decision (mc_plan) depends on the level's shape only, never on the dispatched range.
bool launch_mc_region(McArgs a, int nfaces, hipStream_t st);
// k_mc_region.hip, header 2k: levels up to 16^2 with outputs of 128^2 and more, resident in LDS as a whole; asked ahead of
// launch_mc_region, same contract (pbrk_mc_set_resident)
bool launch_mc_resident(McArgs a, int nfaces, hipStream_t st);

#define MC_MAX_DEVICES 16                           // per-device host state: the k_mc_prep ring, the counters of k_mc_refine_bins
// k_mc_prep.hip: a slot of the scratch ring for one region launch.  words == null: none to be had (mc_plan's have_prep = false).
struct McPrepSlot { unsigned* words = nullptr; int dev = 0, slot = -1; std::unique_lock<std::mutex> hold; };
McPrepSlot mc_prep_acquire(hipStream_t st);
void mc_prep_launch(const McPrepSlot& s, const McArgs& a, const McPlan& p, hipStream_t st);
void mc_prep_release(McPrepSlot& s, hipStream_t st);
