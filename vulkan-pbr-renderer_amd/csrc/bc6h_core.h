// bc6h_core.h -- the one-region search of the BC6H encode contract (K18), written once for the device kernel of k_bc6h.hip and
// for a host compiler: integer arithmetic only, as bc6h_format.h, which holds everything the format fixes (half codes, the scaled
// space, unq, weights, palette).
//
// Output: BC6H_UF16, mode 11 only (mode field 00011): one region, two RGB endpoints of 10 bits each without delta transform, 16 indices
// (3 bits for texel 0, the anchor, 4 bits for every other).  Bits of the little-endian 128-bit block:
//     0-4 mode = 3 | 5-34 r0 g0 b0 | 35-64 r1 g1 b1 | 65-67 index 0 | 68-127 indices 1 .. 15
// Alpha is ignored.  Block texel (x, y) of a level of w x h is the source texel (min(x, w - 1), min(y, h - 1)).
// Endpoint candidates, per block in the scaled space s = (h * 64 + 30) / 31:
//     1. the per-channel bounding box, min -> max on all three channels
//     2. the same box with G resp. B run max -> min where 16 sum(r g) - sum(r) sum(g) resp. the same with b -- 256 times the covariance
//        about the block mean -- is negative (horizon and sunset gradients: red rises as blue falls)
//     3. candidate 2 with both ends of every channel pulled in by (max - min) >> 4
// Each endpoint component is quantised to the x whose bc6h_unq(x, 10) is nearest, the lower x on a tie.  For each candidate texel t
// gets the lowest i that minimises sum_c (palette[i][c] - h_t[c])^2 (at most 3 * 31743^2 < 2^32; the block sum is 64-bit); the
// candidate with the lowest block sum is kept, the earlier one on a tie.  Anchor rule: if the index of texel 0 is 8 or more the
// endpoints are swapped and every i becomes 15 - i (the weights are symmetric: the palette does not change).
#pragma once
#include "bc6h_format.h"

// bc6h_quantize(s, 10) in the spelling this search was first compiled from: the values are equal for every s, but at a constant
// width the compiler turns the shared function into other instructions, and the one-region kernels are held to theirs
// (profiles/bc6h_one_format.md)
BC6H_FN uint32_t bc6h_quantize10(uint32_t s) {
    const uint32_t x1 = s >> 6, x0 = x1 > 0u ? x1 - 1u : 0u, x2 = x1 < 1023u ? x1 + 1u : 1023u;
    const int32_t d0 = (int32_t)bc6h_unq(x0, 10u) - (int32_t)s, d1 = (int32_t)bc6h_unq(x1, 10u) - (int32_t)s, d2 = (int32_t)bc6h_unq(x2, 10u) - (int32_t)s;
    const uint32_t a0 = (uint32_t)(d0 < 0 ? -d0 : d0), a1 = (uint32_t)(d1 < 0 ? -d1 : d1), a2 = (uint32_t)(d2 < 0 ? -d2 : d2);
    uint32_t x = x0, best = a0;
    if (a1 < best) { best = a1; x = x1; }
    if (a2 < best) { x = x2; }
    return x;
}

// One candidate: quantise the endpoints ea / eb (scaled space), give every texel its index; returns the block's squared error.
// q[0..2] = quantised a, q[3..5] = quantised b; idx = 16 indices of 4 bits, texel t at bit 4 t.
BC6H_FN uint64_t bc6h_try(const uint32_t h[16][3], const uint32_t ea[3], const uint32_t eb[3], uint32_t q[6], uint64_t* idx_out) {
    uint32_t ua[3], ub[3];
    BC6H_UNROLL
    for (int c = 0; c < 3; ++c) { q[c] = bc6h_quantize10(ea[c]); q[3 + c] = bc6h_quantize10(eb[c]); ua[c] = bc6h_unq(q[c], 10u); ub[c] = bc6h_unq(q[3 + c], 10u); }
    uint32_t err[16];
    BC6H_UNROLL
    for (int t = 0; t < 16; ++t) err[t] = 0xFFFFFFFFu;
    uint64_t idx = 0;
    BC6H_NO_UNROLL
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t w = bc6h_weight(i);
        const uint32_t p0 = bc6h_palette(ua[0], ub[0], w), p1 = bc6h_palette(ua[1], ub[1], w), p2 = bc6h_palette(ua[2], ub[2], w);
        BC6H_UNROLL
        for (int t = 0; t < 16; ++t) {
            const int32_t d0 = (int32_t)p0 - (int32_t)h[t][0], d1 = (int32_t)p1 - (int32_t)h[t][1], d2 = (int32_t)p2 - (int32_t)h[t][2];
            const uint32_t e = (uint32_t)(d0 * d0) + (uint32_t)(d1 * d1) + (uint32_t)(d2 * d2);
            if (e < err[t]) { err[t] = e; idx = (idx & ~((uint64_t)15u << (4 * t))) | ((uint64_t)i << (4 * t)); }   // strict: the lowest i wins
        }
    }
    uint64_t sum = 0;
    BC6H_UNROLL
    for (int t = 0; t < 16; ++t) sum += err[t];
    *idx_out = idx;
    return sum;
}

// 16 texels (row-major in the block, half codes r g b) -> the block's four little-endian words; returns the block's squared error
BC6H_FN uint64_t bc6h_encode_block_err(const uint32_t h[16][3], uint32_t out[4]) {
    uint32_t lo[3], hi[3], sum[3] = {0, 0, 0};
    uint64_t rg = 0, rb = 0;
    BC6H_UNROLL
    for (int c = 0; c < 3; ++c) { lo[c] = 0xFFFFu; hi[c] = 0u; }
    BC6H_UNROLL
    for (int t = 0; t < 16; ++t) {
        uint32_t s[3];
        BC6H_UNROLL
        for (int c = 0; c < 3; ++c) {
            s[c] = bc6h_scale(h[t][c]);
            lo[c] = s[c] < lo[c] ? s[c] : lo[c];
            hi[c] = s[c] > hi[c] ? s[c] : hi[c];
            sum[c] += s[c];
        }
        rg += (uint64_t)s[0] * s[1];
        rb += (uint64_t)s[0] * s[2];
    }
    // 256 x covariance about the mean; every term is below 2^41
    const bool flip_g = (int64_t)(16u * rg) - (int64_t)((uint64_t)sum[0] * sum[1]) < 0;
    const bool flip_b = (int64_t)(16u * rb) - (int64_t)((uint64_t)sum[0] * sum[2]) < 0;

    uint32_t best_q[6] = {0, 0, 0, 0, 0, 0};
    uint64_t best_idx = 0, best_err = ~(uint64_t)0;
    BC6H_NO_UNROLL
    for (int cand = 0; cand < 3; ++cand) {
        uint32_t ea[3], eb[3];
        BC6H_UNROLL
        for (int c = 0; c < 3; ++c) {
            const uint32_t inset = cand == 2 ? (hi[c] - lo[c]) >> 4 : 0u;
            const bool flip = cand > 0 && ((c == 1 && flip_g) || (c == 2 && flip_b));
            ea[c] = flip ? hi[c] - inset : lo[c] + inset;
            eb[c] = flip ? lo[c] + inset : hi[c] - inset;
        }
        uint32_t q[6];
        uint64_t idx;
        const uint64_t err = bc6h_try(h, ea, eb, q, &idx);
        if (err < best_err) {                                                 // strict: the earlier candidate wins a tie
            best_err = err; best_idx = idx;
            BC6H_UNROLL
            for (int k = 0; k < 6; ++k) best_q[k] = q[k];
        }
    }
    if (best_idx & 8u) {                                                      // anchor rule
        best_idx = ~best_idx;                                                 // 15 - i on every nibble
        BC6H_UNROLL
        for (int c = 0; c < 3; ++c) { const uint32_t t = best_q[c]; best_q[c] = best_q[3 + c]; best_q[3 + c] = t; }
    }
    // pack: 5 + 60 endpoint bits, then index 0 without its top bit, then 15 nibbles
    const uint64_t ends = (uint64_t)best_q[0] | ((uint64_t)best_q[1] << 10) | ((uint64_t)best_q[2] << 20) | ((uint64_t)best_q[3] << 30) |
                          ((uint64_t)best_q[4] << 40) | ((uint64_t)best_q[5] << 50);
    const uint64_t low = 3u | (ends << 5);                                    // bits 0 .. 63; bit 59 of `ends` is block bit 64
    const uint64_t bits63 = (best_idx & 7u) | ((best_idx >> 4) << 3);         // 63 index bits
    const uint64_t high = (ends >> 59) | (bits63 << 1);
    out[0] = (uint32_t)low; out[1] = (uint32_t)(low >> 32); out[2] = (uint32_t)high; out[3] = (uint32_t)(high >> 32);
    return best_err;
}
BC6H_FN void bc6h_encode_block(const uint32_t h[16][3], uint32_t out[4]) { (void)bc6h_encode_block_err(h, out); }
