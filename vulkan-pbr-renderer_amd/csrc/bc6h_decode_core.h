// bc6h_decode_core.h -- the BC6H_UF16 decode contract (K19), written once for the device kernel of k_bc6h_decode.hip and for
// a host compiler (host/pbr_ddsout.c, tests/bc6h_decode_core_host.cpp): integer arithmetic only, so no rounding or denormal mode of
// either machine can change a bit.  tests/bc6h_decode_ref.py restates it in numpy from the format's tables.
//
// A block of 16 bytes (four little-endian words) -> 16 texels x 3 half codes in 0 .. 0x7BFF (never Inf or NaN), row-major in the 4 x 4
// block.  Mode: the low 2 bits if they are 0 or 1, else the low 5 bits; 19, 23, 27 and 31 are reserved and decode to zeros (D3D's rule).
// Each of the 14 modes has its own layout of the endpoint fields (the switch of bc6hd_header: endpoint E of channel c is e[3 E + c],
// field positions are block bits), an endpoint width, three delta widths, and one or two regions; two-region modes carry a 5-bit
// partition at bits 77 .. 81.
//     transformed modes: every endpoint but the base is sign-extended from its channel's delta width, added to the base, masked
//     unquantise at width epb: x for epb >= 15, 0 for 0, 0xFFFF for all ones, else ((x << 15) + 0x4000) >> (epb - 1)
//     one region:  index bits from 65, texel 0 has 3 bits, the others 4; weights bc6h_weight
//     two regions: index bits from 82, texel 0 and the second subset's anchor have 2 bits, the others 3; weights {0, 9, 18, 27, 37,
//                  46, 55, 64}; subset s uses endpoints 2 s and 2 s + 1
//     texel: bc6h_palette(a, b, weight)
// No array is indexed by a run-time value: on the device everything stays in registers.
#pragma once
#include "bc6h_core.h"

typedef struct {
    uint32_t u[12];         // unquantised endpoints, u[3 E + c]
    uint32_t partition;     // 0 .. 31 (two regions)
    uint32_t regions;       // 1, 2; 0: a reserved mode, every texel is zero
} Bc6hdBlock;

// bits pos .. pos + n - 1 of the block, n <= 31; pos and n are constants at every call, so the word index is one too
BC6H_FN uint32_t bc6hd_bits(const uint32_t w[4], uint32_t pos, uint32_t n) {
    const uint32_t i = pos >> 5, s = pos & 31u;
    uint32_t v = w[i] >> s;
    if (s + n > 32u) v |= w[i + 1u] << (32u - s);                             // pos + n <= 128: i + 1 <= 3 here
    return v & ((1u << n) - 1u);
}
BC6H_FN uint32_t bc6hd_rev(uint32_t v, uint32_t n) {                          // the low n bits in reverse order
    uint32_t r = 0;
    BC6H_UNROLL
    for (uint32_t i = 0; i < 6u; ++i) if (i < n) r |= ((v >> i) & 1u) << (n - 1u - i);
    return r;
}
BC6H_FN uint32_t bc6hd_unq(uint32_t x, uint32_t epb) {
    if (epb >= 15u) return x;
    if (x == 0u) return 0u;
    if (x == (1u << epb) - 1u) return 0xFFFFu;
    return ((x << 15) + 0x4000u) >> (epb - 1u);
}
BC6H_FN uint32_t bc6hd_subsets(uint32_t partition) {                          // bit t: texel t belongs to the second subset
    static const uint16_t k[32] = {0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
                                   0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C};
    return k[partition & 31u];
}
BC6H_FN uint32_t bc6hd_anchor(uint32_t partition) {                           // the second subset's anchor texel: 15, 2 or 8
    const uint64_t nibbles = (partition & 16u) ? 0x22882282F882282Full : 0xFFFFFFFFFFFFFFFFull;
    return (uint32_t)(nibbles >> (4u * (partition & 15u))) & 15u;
}
BC6H_FN uint32_t bc6hd_weight3(uint32_t i) { return (i * 64u + 3u) / 7u; }    // {0, 9, 18, 27, 37, 46, 55, 64}

#define BC6HD_CFG(epb, dr, dg, db, transformed, regions) ((epb) | ((dr) << 5) | ((dg) << 9) | ((db) << 13) | ((transformed) << 17) | ((regions) << 18))

// the block's header: mode, endpoint fields, delta transform, unquantisation
BC6H_FN void bc6hd_header(const uint32_t w[4], Bc6hdBlock* b) {
    const uint32_t mode = (w[0] & 3u) < 2u ? (w[0] & 3u) : (w[0] & 31u);
    uint32_t e[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t cfg = 0, part = 0;
    switch (mode) {
    case 0: /* 10; 5,5,5; delta; 2 */
        e[7] |= bc6hd_bits(w, 2, 1) << 4; e[8] |= bc6hd_bits(w, 3, 1) << 4; e[11] |= bc6hd_bits(w, 4, 1) << 4; e[0] |= bc6hd_bits(w, 5, 10);
        e[1] |= bc6hd_bits(w, 15, 10); e[2] |= bc6hd_bits(w, 25, 10); e[3] |= bc6hd_bits(w, 35, 5); e[10] |= bc6hd_bits(w, 40, 1) << 4;
        e[7] |= bc6hd_bits(w, 41, 4); e[4] |= bc6hd_bits(w, 45, 5); e[11] |= bc6hd_bits(w, 50, 1); e[10] |= bc6hd_bits(w, 51, 4);
        e[5] |= bc6hd_bits(w, 55, 5); e[11] |= bc6hd_bits(w, 60, 1) << 1; e[8] |= bc6hd_bits(w, 61, 4); e[6] |= bc6hd_bits(w, 65, 5);
        e[11] |= bc6hd_bits(w, 70, 1) << 2; e[9] |= bc6hd_bits(w, 71, 5); e[11] |= bc6hd_bits(w, 76, 1) << 3; part = bc6hd_bits(w, 77, 5);
        cfg = BC6HD_CFG(10, 5, 5, 5, 1, 2); break;
    case 1: /* 7; 6,6,6; delta; 2 */
        e[7] |= bc6hd_bits(w, 2, 1) << 5; e[10] |= bc6hd_bits(w, 3, 1) << 4; e[10] |= bc6hd_bits(w, 4, 1) << 5; e[0] |= bc6hd_bits(w, 5, 7);
        e[11] |= bc6hd_bits(w, 12, 1); e[11] |= bc6hd_bits(w, 13, 1) << 1; e[8] |= bc6hd_bits(w, 14, 1) << 4; e[1] |= bc6hd_bits(w, 15, 7);
        e[8] |= bc6hd_bits(w, 22, 1) << 5; e[11] |= bc6hd_bits(w, 23, 1) << 2; e[7] |= bc6hd_bits(w, 24, 1) << 4; e[2] |= bc6hd_bits(w, 25, 7);
        e[11] |= bc6hd_bits(w, 32, 1) << 3; e[11] |= bc6hd_bits(w, 33, 1) << 5; e[11] |= bc6hd_bits(w, 34, 1) << 4; e[3] |= bc6hd_bits(w, 35, 6);
        e[7] |= bc6hd_bits(w, 41, 4); e[4] |= bc6hd_bits(w, 45, 6); e[10] |= bc6hd_bits(w, 51, 4); e[5] |= bc6hd_bits(w, 55, 6);
        e[8] |= bc6hd_bits(w, 61, 4); e[6] |= bc6hd_bits(w, 65, 6); e[9] |= bc6hd_bits(w, 71, 6); part = bc6hd_bits(w, 77, 5);
        cfg = BC6HD_CFG(7, 6, 6, 6, 1, 2); break;
    case 2: /* 11; 5,4,4; delta; 2 */
        e[0] |= bc6hd_bits(w, 5, 10); e[1] |= bc6hd_bits(w, 15, 10); e[2] |= bc6hd_bits(w, 25, 10); e[3] |= bc6hd_bits(w, 35, 5);
        e[0] |= bc6hd_bits(w, 40, 1) << 10; e[7] |= bc6hd_bits(w, 41, 4); e[4] |= bc6hd_bits(w, 45, 4); e[1] |= bc6hd_bits(w, 49, 1) << 10;
        e[11] |= bc6hd_bits(w, 50, 1); e[10] |= bc6hd_bits(w, 51, 4); e[5] |= bc6hd_bits(w, 55, 4); e[2] |= bc6hd_bits(w, 59, 1) << 10;
        e[11] |= bc6hd_bits(w, 60, 1) << 1; e[8] |= bc6hd_bits(w, 61, 4); e[6] |= bc6hd_bits(w, 65, 5); e[11] |= bc6hd_bits(w, 70, 1) << 2;
        e[9] |= bc6hd_bits(w, 71, 5); e[11] |= bc6hd_bits(w, 76, 1) << 3; part = bc6hd_bits(w, 77, 5);
        cfg = BC6HD_CFG(11, 5, 4, 4, 1, 2); break;
    case 3: /* 10; 10,10,10; plain; 1 */
        e[0] |= bc6hd_bits(w, 5, 10); e[1] |= bc6hd_bits(w, 15, 10); e[2] |= bc6hd_bits(w, 25, 10); e[3] |= bc6hd_bits(w, 35, 10);
        e[4] |= bc6hd_bits(w, 45, 10); e[5] |= bc6hd_bits(w, 55, 10);
        cfg = BC6HD_CFG(10, 10, 10, 10, 0, 1); break;
    case 6: /* 11; 4,5,4; delta; 2 */
        e[0] |= bc6hd_bits(w, 5, 10); e[1] |= bc6hd_bits(w, 15, 10); e[2] |= bc6hd_bits(w, 25, 10); e[3] |= bc6hd_bits(w, 35, 4);
        e[0] |= bc6hd_bits(w, 39, 1) << 10; e[10] |= bc6hd_bits(w, 40, 1) << 4; e[7] |= bc6hd_bits(w, 41, 4); e[4] |= bc6hd_bits(w, 45, 5);
        e[1] |= bc6hd_bits(w, 50, 1) << 10; e[10] |= bc6hd_bits(w, 51, 4); e[5] |= bc6hd_bits(w, 55, 4); e[2] |= bc6hd_bits(w, 59, 1) << 10;
        e[11] |= bc6hd_bits(w, 60, 1) << 1; e[8] |= bc6hd_bits(w, 61, 4); e[6] |= bc6hd_bits(w, 65, 4); e[11] |= bc6hd_bits(w, 69, 1);
        e[11] |= bc6hd_bits(w, 70, 1) << 2; e[9] |= bc6hd_bits(w, 71, 4); e[7] |= bc6hd_bits(w, 75, 1) << 4; e[11] |= bc6hd_bits(w, 76, 1) << 3;
        part = bc6hd_bits(w, 77, 5);
        cfg = BC6HD_CFG(11, 4, 5, 4, 1, 2); break;
    case 7: /* 11; 9,9,9; delta; 1 */
        e[0] |= bc6hd_bits(w, 5, 10); e[1] |= bc6hd_bits(w, 15, 10); e[2] |= bc6hd_bits(w, 25, 10); e[3] |= bc6hd_bits(w, 35, 9);
        e[0] |= bc6hd_bits(w, 44, 1) << 10; e[4] |= bc6hd_bits(w, 45, 9); e[1] |= bc6hd_bits(w, 54, 1) << 10; e[5] |= bc6hd_bits(w, 55, 9);
        e[2] |= bc6hd_bits(w, 64, 1) << 10;
        cfg = BC6HD_CFG(11, 9, 9, 9, 1, 1); break;
    case 10: /* 11; 4,4,5; delta; 2 */
        e[0] |= bc6hd_bits(w, 5, 10); e[1] |= bc6hd_bits(w, 15, 10); e[2] |= bc6hd_bits(w, 25, 10); e[3] |= bc6hd_bits(w, 35, 4);
        e[0] |= bc6hd_bits(w, 39, 1) << 10; e[8] |= bc6hd_bits(w, 40, 1) << 4; e[7] |= bc6hd_bits(w, 41, 4); e[4] |= bc6hd_bits(w, 45, 4);
        e[1] |= bc6hd_bits(w, 49, 1) << 10; e[11] |= bc6hd_bits(w, 50, 1); e[10] |= bc6hd_bits(w, 51, 4); e[5] |= bc6hd_bits(w, 55, 5);
        e[2] |= bc6hd_bits(w, 60, 1) << 10; e[8] |= bc6hd_bits(w, 61, 4); e[6] |= bc6hd_bits(w, 65, 4); e[11] |= bc6hd_bits(w, 69, 1) << 1;
        e[11] |= bc6hd_bits(w, 70, 1) << 2; e[9] |= bc6hd_bits(w, 71, 4); e[11] |= bc6hd_bits(w, 75, 1) << 4; e[11] |= bc6hd_bits(w, 76, 1) << 3;
        part = bc6hd_bits(w, 77, 5);
        cfg = BC6HD_CFG(11, 4, 4, 5, 1, 2); break;
    case 11: /* 12; 8,8,8; delta; 1 */
        e[0] |= bc6hd_bits(w, 5, 10); e[1] |= bc6hd_bits(w, 15, 10); e[2] |= bc6hd_bits(w, 25, 10); e[3] |= bc6hd_bits(w, 35, 8);
        e[0] |= bc6hd_rev(bc6hd_bits(w, 43, 2), 2) << 10; e[4] |= bc6hd_bits(w, 45, 8); e[1] |= bc6hd_rev(bc6hd_bits(w, 53, 2), 2) << 10;
        e[5] |= bc6hd_bits(w, 55, 8); e[2] |= bc6hd_rev(bc6hd_bits(w, 63, 2), 2) << 10;
        cfg = BC6HD_CFG(12, 8, 8, 8, 1, 1); break;
    case 14: /* 9; 5,5,5; delta; 2 */
        e[0] |= bc6hd_bits(w, 5, 9); e[8] |= bc6hd_bits(w, 14, 1) << 4; e[1] |= bc6hd_bits(w, 15, 9); e[7] |= bc6hd_bits(w, 24, 1) << 4;
        e[2] |= bc6hd_bits(w, 25, 9); e[11] |= bc6hd_bits(w, 34, 1) << 4; e[3] |= bc6hd_bits(w, 35, 5); e[10] |= bc6hd_bits(w, 40, 1) << 4;
        e[7] |= bc6hd_bits(w, 41, 4); e[4] |= bc6hd_bits(w, 45, 5); e[11] |= bc6hd_bits(w, 50, 1); e[10] |= bc6hd_bits(w, 51, 4);
        e[5] |= bc6hd_bits(w, 55, 5); e[11] |= bc6hd_bits(w, 60, 1) << 1; e[8] |= bc6hd_bits(w, 61, 4); e[6] |= bc6hd_bits(w, 65, 5);
        e[11] |= bc6hd_bits(w, 70, 1) << 2; e[9] |= bc6hd_bits(w, 71, 5); e[11] |= bc6hd_bits(w, 76, 1) << 3; part = bc6hd_bits(w, 77, 5);
        cfg = BC6HD_CFG(9, 5, 5, 5, 1, 2); break;
    case 15: /* 16; 4,4,4; delta; 1 */
        e[0] |= bc6hd_bits(w, 5, 10); e[1] |= bc6hd_bits(w, 15, 10); e[2] |= bc6hd_bits(w, 25, 10); e[3] |= bc6hd_bits(w, 35, 4);
        e[0] |= bc6hd_rev(bc6hd_bits(w, 39, 6), 6) << 10; e[4] |= bc6hd_bits(w, 45, 4); e[1] |= bc6hd_rev(bc6hd_bits(w, 49, 6), 6) << 10;
        e[5] |= bc6hd_bits(w, 55, 4); e[2] |= bc6hd_rev(bc6hd_bits(w, 59, 6), 6) << 10;
        cfg = BC6HD_CFG(16, 4, 4, 4, 1, 1); break;
    case 18: /* 8; 6,5,5; delta; 2 */
        e[0] |= bc6hd_bits(w, 5, 8); e[10] |= bc6hd_bits(w, 13, 1) << 4; e[8] |= bc6hd_bits(w, 14, 1) << 4; e[1] |= bc6hd_bits(w, 15, 8);
        e[11] |= bc6hd_bits(w, 23, 1) << 2; e[7] |= bc6hd_bits(w, 24, 1) << 4; e[2] |= bc6hd_bits(w, 25, 8); e[11] |= bc6hd_bits(w, 33, 1) << 3;
        e[11] |= bc6hd_bits(w, 34, 1) << 4; e[3] |= bc6hd_bits(w, 35, 6); e[7] |= bc6hd_bits(w, 41, 4); e[4] |= bc6hd_bits(w, 45, 5);
        e[11] |= bc6hd_bits(w, 50, 1); e[10] |= bc6hd_bits(w, 51, 4); e[5] |= bc6hd_bits(w, 55, 5); e[11] |= bc6hd_bits(w, 60, 1) << 1;
        e[8] |= bc6hd_bits(w, 61, 4); e[6] |= bc6hd_bits(w, 65, 6); e[9] |= bc6hd_bits(w, 71, 6); part = bc6hd_bits(w, 77, 5);
        cfg = BC6HD_CFG(8, 6, 5, 5, 1, 2); break;
    case 22: /* 8; 5,6,5; delta; 2 */
        e[0] |= bc6hd_bits(w, 5, 8); e[11] |= bc6hd_bits(w, 13, 1); e[8] |= bc6hd_bits(w, 14, 1) << 4; e[1] |= bc6hd_bits(w, 15, 8);
        e[7] |= bc6hd_bits(w, 23, 1) << 5; e[7] |= bc6hd_bits(w, 24, 1) << 4; e[2] |= bc6hd_bits(w, 25, 8); e[10] |= bc6hd_bits(w, 33, 1) << 5;
        e[11] |= bc6hd_bits(w, 34, 1) << 4; e[3] |= bc6hd_bits(w, 35, 5); e[10] |= bc6hd_bits(w, 40, 1) << 4; e[7] |= bc6hd_bits(w, 41, 4);
        e[4] |= bc6hd_bits(w, 45, 6); e[10] |= bc6hd_bits(w, 51, 4); e[5] |= bc6hd_bits(w, 55, 5); e[11] |= bc6hd_bits(w, 60, 1) << 1;
        e[8] |= bc6hd_bits(w, 61, 4); e[6] |= bc6hd_bits(w, 65, 5); e[11] |= bc6hd_bits(w, 70, 1) << 2; e[9] |= bc6hd_bits(w, 71, 5);
        e[11] |= bc6hd_bits(w, 76, 1) << 3; part = bc6hd_bits(w, 77, 5);
        cfg = BC6HD_CFG(8, 5, 6, 5, 1, 2); break;
    case 26: /* 8; 5,5,6; delta; 2 */
        e[0] |= bc6hd_bits(w, 5, 8); e[11] |= bc6hd_bits(w, 13, 1) << 1; e[8] |= bc6hd_bits(w, 14, 1) << 4; e[1] |= bc6hd_bits(w, 15, 8);
        e[8] |= bc6hd_bits(w, 23, 1) << 5; e[7] |= bc6hd_bits(w, 24, 1) << 4; e[2] |= bc6hd_bits(w, 25, 8); e[11] |= bc6hd_bits(w, 33, 1) << 5;
        e[11] |= bc6hd_bits(w, 34, 1) << 4; e[3] |= bc6hd_bits(w, 35, 5); e[10] |= bc6hd_bits(w, 40, 1) << 4; e[7] |= bc6hd_bits(w, 41, 4);
        e[4] |= bc6hd_bits(w, 45, 5); e[11] |= bc6hd_bits(w, 50, 1); e[10] |= bc6hd_bits(w, 51, 4); e[5] |= bc6hd_bits(w, 55, 6);
        e[8] |= bc6hd_bits(w, 61, 4); e[6] |= bc6hd_bits(w, 65, 5); e[11] |= bc6hd_bits(w, 70, 1) << 2; e[9] |= bc6hd_bits(w, 71, 5);
        e[11] |= bc6hd_bits(w, 76, 1) << 3; part = bc6hd_bits(w, 77, 5);
        cfg = BC6HD_CFG(8, 5, 5, 6, 1, 2); break;
    case 30: /* 6; 6,6,6; plain; 2 */
        e[0] |= bc6hd_bits(w, 5, 6); e[10] |= bc6hd_bits(w, 11, 1) << 4; e[11] |= bc6hd_bits(w, 12, 1); e[11] |= bc6hd_bits(w, 13, 1) << 1;
        e[8] |= bc6hd_bits(w, 14, 1) << 4; e[1] |= bc6hd_bits(w, 15, 6); e[7] |= bc6hd_bits(w, 21, 1) << 5; e[8] |= bc6hd_bits(w, 22, 1) << 5;
        e[11] |= bc6hd_bits(w, 23, 1) << 2; e[7] |= bc6hd_bits(w, 24, 1) << 4; e[2] |= bc6hd_bits(w, 25, 6); e[10] |= bc6hd_bits(w, 31, 1) << 5;
        e[11] |= bc6hd_bits(w, 32, 1) << 3; e[11] |= bc6hd_bits(w, 33, 1) << 5; e[11] |= bc6hd_bits(w, 34, 1) << 4; e[3] |= bc6hd_bits(w, 35, 6);
        e[7] |= bc6hd_bits(w, 41, 4); e[4] |= bc6hd_bits(w, 45, 6); e[10] |= bc6hd_bits(w, 51, 4); e[5] |= bc6hd_bits(w, 55, 6);
        e[8] |= bc6hd_bits(w, 61, 4); e[6] |= bc6hd_bits(w, 65, 6); e[9] |= bc6hd_bits(w, 71, 6); part = bc6hd_bits(w, 77, 5);
        cfg = BC6HD_CFG(6, 6, 6, 6, 0, 2); break;
    default: break;                                                           /* 19, 23, 27, 31: reserved */
    }
    const uint32_t epb = cfg & 31u, regions = cfg >> 18, mask = epb ? (0xFFFFFFFFu >> (32u - epb)) : 0u;
    if (cfg & (1u << 17)) {
        BC6H_UNROLL
        for (int c = 0; c < 3; ++c) {
            const uint32_t up = 32u - ((cfg >> (5 + 4 * c)) & 15u);           // sign extension from the channel's delta width
            BC6H_UNROLL
            for (int k = 1; k < 4; ++k) e[3 * k + c] = (e[c] + (uint32_t)((int32_t)(e[3 * k + c] << up) >> up)) & mask;
        }
    }
    BC6H_UNROLL
    for (int i = 0; i < 12; ++i) b->u[i] = regions ? bc6hd_unq(e[i], epb) : 0u;
    b->partition = part;
    b->regions = regions;
}

// texel t (0 .. 15, row-major) of a block whose header is b
BC6H_FN void bc6hd_texel(const Bc6hdBlock* b, const uint32_t w[4], uint32_t t, uint32_t rgb[3]) {
    const uint64_t hi = (uint64_t)w[2] | ((uint64_t)w[3] << 32);              // block bits 64 .. 127: every index bit
    uint32_t weight, second = 0;
    if (b->regions == 2u) {
        const uint32_t anchor = bc6hd_anchor(b->partition);
        const uint32_t pos = 18u + 3u * t - (t > 0u ? 1u : 0u) - (t > anchor ? 1u : 0u), n = (t == 0u || t == anchor) ? 2u : 3u;
        weight = bc6hd_weight3((uint32_t)(hi >> pos) & ((1u << n) - 1u));
        second = (bc6hd_subsets(b->partition) >> t) & 1u;
    } else {
        const uint32_t pos = t == 0u ? 1u : 4u * t, n = t == 0u ? 3u : 4u;
        weight = bc6h_weight((uint32_t)(hi >> pos) & ((1u << n) - 1u));
    }
    BC6H_UNROLL
    for (int c = 0; c < 3; ++c) {
        const uint32_t lo = second ? b->u[6 + c] : b->u[c], up = second ? b->u[9 + c] : b->u[3 + c];
        rgb[c] = b->regions ? bc6h_palette(lo, up, weight) : 0u;
    }
}

// row `row` (0 .. 3) of the block: four texels
BC6H_FN void bc6hd_decode_row(const uint32_t w[4], uint32_t row, uint32_t rgb[4][3]) {
    Bc6hdBlock b;
    bc6hd_header(w, &b);
    BC6H_UNROLL
    for (uint32_t x = 0; x < 4u; ++x) bc6hd_texel(&b, w, 4u * row + x, rgb[x]);
}
BC6H_FN void bc6hd_decode_block(const uint32_t w[4], uint32_t rgb[16][3]) {
    Bc6hdBlock b;
    bc6hd_header(w, &b);
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; ++t) bc6hd_texel(&b, w, t, rgb[t]);
}

// half code 0 .. 0x7BFF -> the fp32 bits of the same value: the exact widening, subnormal halves included, in integers
BC6H_FN uint32_t bc6hd_f32_from_code(uint32_t h) {
    if (h >= 0x400u) return (h << 13) + (112u << 23);
    if (h == 0u) return 0u;
    const uint32_t p = 31u - (uint32_t)__builtin_clz(h);                      // h 2^-24 = 1.m x 2^(p - 24), p = 0 .. 9
    return ((p + 103u) << 23) | ((h << (23u - p)) & 0x7FFFFFu);
}
