// bc6h2_core.h -- the two-region quality level of the BC6H encode contract (K18, DESIGN.md "K18, two regions"), written once for the
// device kernel of k_bc6h.hip and for a host compiler (tests/bc6h_encode_host.cpp): integer arithmetic only, as bc6h_core.h.
// tests/bc6h2_ref.py restates it in numpy.
//
// Output: BC6H_UF16, per block either the one-region block of bc6h_core.h (mode 11, mode field 00011) or one of the four symmetric
// two-region modes, named by their mode field as the lists of bc6h_format.h:
//     case  0: endpoints of 10 bits, deltas of 5     case 14: 9 bits, deltas of 5
//     case  1:  7 bits, deltas of 6                  case 30: 6 bits, no delta transform
// 1. The one-region block and its squared error E1 are bc6h_encode_block_err's.  E1 = 0 ends the block there.
// 2. For every partition p = 0 .. 31 in ascending order, for each of its two subsets (bit t of bc6hd_subsets(p): texel t, row-major,
//    belongs to subset 1): in the scaled space s = bc6h_scale(h) take the per-channel bounding box of the subset's texels, min -> max,
//    with G resp. B run max -> min where n sum(r c) - sum(r) sum(c) < 0 over the subset (n its texel count): candidate 2 of the
//    one-region rule per subset, without an inset.  Four endpoints a0, b0 (subset 0), a1, b1 (subset 1).
// 3. The mode of the partition is the first of case 0, 14, 1, 30 that fits.  All four endpoints are quantised at the mode's width epb:
//    the x whose bc6h_unq(x, epb) is nearest, the lower x on a tie (bc6h_quantize).  A delta mode fits when in every channel max - min
//    over the four quantised endpoints is <= 2^(d - 1) - 1 (15 resp. 31): whichever endpoint becomes the base, every difference then
//    fits d signed bits.  Case 30 always fits.
// 4. Texel t gets the lowest i in 0 .. 7 that minimises sum_c (palette - h)^2, the palette being bc6h_palette(ua, ub, bc6hd_weight3(i))
//    of its own subset's unquantised endpoints.  E2(p) is the sum of those minima (64-bit).  The partition with the lowest E2 wins, the
//    lower p on a tie, and the two-region block replaces the one-region block only if E2 < E1.
// 5. Anchors: texel 0 for subset 0, bc6hd_anchor(p) for subset 1.  If a subset's anchor index is 4 or more that subset's endpoints are
//    swapped and every index of its texels becomes 7 - i (the weights are symmetric: the palette does not change).  Then e0, e1 = subset
//    0's pair, e2, e3 = subset 1's; in the delta modes e1 .. e3 are stored as (e_k - e0) masked to d bits.
// 6. Packing: the mode's field list of bc6h_format.h expanded with the writer, the partition at bits 77 .. 81, indices from bit 82 in
//    texel order, 2 bits for the two anchors and 3 for every other texel.
// The partition loop is rolled (p and the subset mask are the same for every block in flight: scalars on the device), the loops over
// texels and channels are unrolled, so no array is indexed by a run-time value.
#pragma once
#include "bc6h_core.h"

// what was chosen for a block; the tests read it, the kernel drops it
typedef struct {
    uint32_t kind;          // 0: one region; 1, 2, 3, 4: case 0, 14, 1, 30
    uint32_t partition;     // 0 .. 31 (two regions)
    uint64_t err;           // the block's squared half-code error
} Bc6h2Info;

BC6H_FN uint32_t bc6h2_epb(uint32_t m) { return m == 0u ? 10u : m == 1u ? 9u : m == 2u ? 7u : 6u; }   // m: 0, 1, 2, 3 = case 0, 14, 1, 30

// One partition (steps 2 .. 4).  hs[t][c] = half code | scaled value << 16; mask = bc6hd_subsets(p).  q[3 E + c] = the quantised
// endpoints a0, b0, a1, b1; *m_out = the mode; idx = 16 indices, texel t at bit 4 t.  Returns E2.
BC6H_FN uint64_t bc6h2_try(const uint32_t hs[16][3], uint32_t mask, uint32_t q[12], uint32_t* m_out, uint64_t* idx_out) {
    uint32_t lo[2][3], hi[2][3], sum[2][3];
    uint64_t rg[2] = {0, 0}, rb[2] = {0, 0};
    BC6H_UNROLL
    for (int k = 0; k < 2; ++k) {
        BC6H_UNROLL
        for (int c = 0; c < 3; ++c) { lo[k][c] = 0xFFFFu; hi[k][c] = 0u; sum[k][c] = 0u; }
    }
    BC6H_UNROLL
    for (int t = 0; t < 16; ++t) {
        const bool in1 = ((mask >> t) & 1u) != 0u;
        const uint32_t s0 = hs[t][0] >> 16, s1 = hs[t][1] >> 16, s2 = hs[t][2] >> 16;
        BC6H_UNROLL
        for (int k = 0; k < 2; ++k) {
            const bool on = in1 == (k == 1);
            BC6H_UNROLL
            for (int c = 0; c < 3; ++c) {
                const uint32_t s = hs[t][c] >> 16;
                lo[k][c] = on && s < lo[k][c] ? s : lo[k][c];
                hi[k][c] = on && s > hi[k][c] ? s : hi[k][c];
                sum[k][c] += on ? s : 0u;
            }
            rg[k] += on ? (uint64_t)s0 * s1 : 0u;
            rb[k] += on ? (uint64_t)s0 * s2 : 0u;
        }
    }
    const uint32_t n1 = (uint32_t)__builtin_popcount(mask & 0xFFFFu);
    uint32_t sp[12];                                                          // a0 b0 a1 b1 in the scaled space
    BC6H_UNROLL
    for (int k = 0; k < 2; ++k) {
        const uint64_t n = k ? n1 : 16u - n1;                                 // every term is below 2^41
        const bool flip_g = (int64_t)(n * rg[k]) - (int64_t)((uint64_t)sum[k][0] * sum[k][1]) < 0;
        const bool flip_b = (int64_t)(n * rb[k]) - (int64_t)((uint64_t)sum[k][0] * sum[k][2]) < 0;
        BC6H_UNROLL
        for (int c = 0; c < 3; ++c) {
            const bool flip = (c == 1 && flip_g) || (c == 2 && flip_b);
            sp[6 * k + c] = flip ? hi[k][c] : lo[k][c];
            sp[6 * k + 3 + c] = flip ? lo[k][c] : hi[k][c];
        }
    }
    uint32_t m = 0, epb = 10;
    BC6H_NO_UNROLL
    for (;; ++m) {                                                            // step 3: the first mode that fits
        epb = bc6h2_epb(m);
        BC6H_UNROLL
        for (int i = 0; i < 12; ++i) q[i] = bc6h_quantize(sp[i], epb);
        if (m == 3u) break;
        const uint32_t limit = m == 2u ? 31u : 15u;
        bool fit = true;
        BC6H_UNROLL
        for (int c = 0; c < 3; ++c) {
            uint32_t mn = q[c], mx = q[c];
            BC6H_UNROLL
            for (int e = 1; e < 4; ++e) { mn = q[3 * e + c] < mn ? q[3 * e + c] : mn; mx = q[3 * e + c] > mx ? q[3 * e + c] : mx; }
            fit = fit && mx - mn <= limit;
        }
        if (fit) break;
    }
    uint32_t u[12], err[16];
    BC6H_UNROLL
    for (int i = 0; i < 12; ++i) u[i] = bc6h_unq(q[i], epb);
    BC6H_UNROLL
    for (int t = 0; t < 16; ++t) err[t] = 0xFFFFFFFFu;
    uint64_t idx = 0;
    BC6H_NO_UNROLL
    for (uint32_t i = 0; i < 8u; ++i) {
        const uint32_t w = bc6hd_weight3(i);
        uint32_t pal[2][3];
        BC6H_UNROLL
        for (int k = 0; k < 2; ++k) {
            BC6H_UNROLL
            for (int c = 0; c < 3; ++c) pal[k][c] = bc6h_palette(u[6 * k + c], u[6 * k + 3 + c], w);
        }
        BC6H_UNROLL
        for (int t = 0; t < 16; ++t) {
            const bool in1 = ((mask >> t) & 1u) != 0u;
            const int32_t d0 = (int32_t)(in1 ? pal[1][0] : pal[0][0]) - (int32_t)(hs[t][0] & 0xFFFFu);
            const int32_t d1 = (int32_t)(in1 ? pal[1][1] : pal[0][1]) - (int32_t)(hs[t][1] & 0xFFFFu);
            const int32_t d2 = (int32_t)(in1 ? pal[1][2] : pal[0][2]) - (int32_t)(hs[t][2] & 0xFFFFu);
            const uint32_t e = (uint32_t)(d0 * d0) + (uint32_t)(d1 * d1) + (uint32_t)(d2 * d2);   // at most 3 * 31743^2 < 2^32
            if (e < err[t]) { err[t] = e; idx = (idx & ~((uint64_t)15u << (4 * t))) | ((uint64_t)i << (4 * t)); }   // strict: the lowest i wins
        }
    }
    uint64_t total = 0;
    BC6H_UNROLL
    for (int t = 0; t < 16; ++t) total += err[t];
    *m_out = m;
    *idx_out = idx;
    return total;
}

// step 6: e[3 E + c] as the field lists name them (e1 .. e3 already deltas where the mode has them), indices after the anchor rule
BC6H_FN void bc6h2_pack(uint32_t m, const uint32_t e[12], uint32_t partition, uint64_t idx, uint32_t out[4]) {
    uint32_t w[4] = {0, 0, 0, 0};
    if (m == 0u) { BC6H_MODE0(BC6H_PUT) }
    else if (m == 1u) { w[0] = 14u; BC6H_MODE14(BC6H_PUT) }
    else if (m == 2u) { w[0] = 1u; BC6H_MODE1(BC6H_PUT) }
    else { w[0] = 30u; BC6H_MODE30(BC6H_PUT) }
    bc6h_put_bits(w, 77, 5, partition);
    const uint32_t anchor = bc6hd_anchor(partition);
    uint64_t bits = 0;                                                        // the 46 index bits, block bit 82 at bit 0
    uint32_t pos = 0;
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; ++t) {
        bits |= ((idx >> (4u * t)) & 7u) << pos;                              // an anchor's index is below 4: its top bit is not stored
        pos += (t == 0u || t == anchor) ? 2u : 3u;
    }
    const uint64_t high = (uint64_t)w[2] | ((uint64_t)w[3] << 32) | (bits << 18);
    out[0] = w[0]; out[1] = w[1]; out[2] = (uint32_t)high; out[3] = (uint32_t)(high >> 32);
}

// 16 texels (row-major in the block, half codes r g b) -> the block's four little-endian words, and what was chosen
BC6H_FN void bc6h2_encode_block(const uint32_t h[16][3], uint32_t out[4], Bc6h2Info* info) {
    const uint64_t e1 = bc6h_encode_block_err(h, out);
    info->kind = 0u; info->partition = 0u; info->err = e1;
    if (e1 == 0u) return;                                                     // nothing can be strictly better
    uint32_t hs[16][3];
    BC6H_UNROLL
    for (int t = 0; t < 16; ++t) {
        BC6H_UNROLL
        for (int c = 0; c < 3; ++c) hs[t][c] = h[t][c] | (bc6h_scale(h[t][c]) << 16);   // 15 and 16 bits
    }
    uint32_t best_q[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, best_m = 0, best_p = 32u;
    uint64_t best_idx = 0, best_err = e1;
    BC6H_NO_UNROLL
    for (uint32_t p = 0; p < 32u; ++p) {
        uint32_t q[12], m;
        uint64_t idx;
        const uint64_t err = bc6h2_try(hs, bc6hd_subsets(p), q, &m, &idx);
        if (err < best_err) {                                                 // strict: the one-region block, then the lower p, wins a tie
            best_err = err; best_idx = idx; best_m = m; best_p = p;
            BC6H_UNROLL
            for (int i = 0; i < 12; ++i) best_q[i] = q[i];
        }
    }
    if (best_p == 32u) return;
    // step 5: the anchor rule per subset
    const uint32_t mask = bc6hd_subsets(best_p), anchor = bc6hd_anchor(best_p);
    const bool swap0 = (best_idx & 4u) != 0u, swap1 = ((best_idx >> (4u * anchor)) & 4u) != 0u;
    uint64_t invert = 0;
    BC6H_UNROLL
    for (int t = 0; t < 16; ++t) invert |= (((mask >> t) & 1u) ? swap1 : swap0) ? (uint64_t)7u << (4 * t) : 0u;
    best_idx ^= invert;                                                       // 7 - i on every index of a swapped subset
    BC6H_UNROLL
    for (int c = 0; c < 3; ++c) {
        if (swap0) { const uint32_t t = best_q[c]; best_q[c] = best_q[3 + c]; best_q[3 + c] = t; }
        if (swap1) { const uint32_t t = best_q[6 + c]; best_q[6 + c] = best_q[9 + c]; best_q[9 + c] = t; }
    }
    uint32_t e[12];
    const uint32_t dmask = best_m == 3u ? 0xFFFFFFFFu : best_m == 2u ? 63u : 31u;
    BC6H_UNROLL
    for (int i = 0; i < 12; ++i) e[i] = i < 3 ? best_q[i] : best_m == 3u ? best_q[i] : (best_q[i] - best_q[i % 3]) & dmask;
    bc6h2_pack(best_m, e, best_p, best_idx, out);
    info->kind = best_m + 1u; info->partition = best_p; info->err = best_err;
}
