// bc6h_decode_core.h -- the BC6H_UF16 decode contract (K19), written once for the device kernel of k_bc6h_decode.hip and for
// a host compiler (host/pbr_ddsin.c, tests/bc6h_decode_core_host.cpp): integer arithmetic only, as bc6h_format.h, which holds the
// format's tables and the field lists of the 14 modes.  tests/bc6h_decode_ref.py restates it in numpy from the format's tables.
//
// A block of 16 bytes (four little-endian words) -> 16 texels x 3 half codes in 0 .. 0x7BFF (never Inf or NaN), row-major in the 4 x 4
// block.  Mode: the low 2 bits if they are 0 or 1, else the low 5 bits; 19, 23, 27 and 31 are reserved and decode to zeros (D3D's rule).
// Each of the 14 modes has its own layout of the endpoint fields (its list in bc6h_format.h: endpoint E of channel c is e[3 E + c]),
// an endpoint width, three delta widths, and one or two regions; two-region modes carry a 5-bit partition at bits 77 .. 81.
//     transformed modes: every endpoint but the base is sign-extended from its channel's delta width, added to the base, masked
//     unquantise at width epb: bc6h_unq
//     one region:  index bits from 65, texel 0 has 3 bits, the others 4; weights bc6h_weight
//     two regions: index bits from 82, texel 0 and the second subset's anchor have 2 bits, the others 3; weights bc6hd_weight3;
//                  subset s uses endpoints 2 s and 2 s + 1
//     texel: bc6h_palette(a, b, weight)
// No array is indexed by a run-time value: on the device everything stays in registers.
#pragma once
#include "bc6h_format.h"

typedef struct {
    uint32_t u[12];         // unquantised endpoints, u[3 E + c]
    uint32_t partition;     // 0 .. 31 (two regions)
    uint32_t regions;       // 1, 2; 0: a reserved mode, every texel is zero
} Bc6hdBlock;

#define BC6HD_CFG(epb, dr, dg, db, transformed, regions) ((epb) | ((dr) << 5) | ((dg) << 9) | ((db) << 13) | ((transformed) << 17) | ((regions) << 18))

// the block's header: mode, endpoint fields, delta transform, unquantisation
BC6H_FN void bc6hd_header(const uint32_t w[4], Bc6hdBlock* b) {
    const uint32_t mode = (w[0] & 3u) < 2u ? (w[0] & 3u) : (w[0] & 31u);
    uint32_t e[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t cfg = 0, part = 0;
    switch (mode) {
    case 0: /* 10; 5,5,5; delta; 2 */ BC6H_MODE0(BC6H_GET) part = bc6hd_bits(w, 77, 5); cfg = BC6HD_CFG(10, 5, 5, 5, 1, 2); break;
    case 1: /* 7; 6,6,6; delta; 2 */ BC6H_MODE1(BC6H_GET) part = bc6hd_bits(w, 77, 5); cfg = BC6HD_CFG(7, 6, 6, 6, 1, 2); break;
    case 2: /* 11; 5,4,4; delta; 2 */ BC6H_MODE2(BC6H_GET) part = bc6hd_bits(w, 77, 5); cfg = BC6HD_CFG(11, 5, 4, 4, 1, 2); break;
    case 3: /* 10; 10,10,10; plain; 1 */ BC6H_MODE3(BC6H_GET) cfg = BC6HD_CFG(10, 10, 10, 10, 0, 1); break;
    case 6: /* 11; 4,5,4; delta; 2 */ BC6H_MODE6(BC6H_GET) part = bc6hd_bits(w, 77, 5); cfg = BC6HD_CFG(11, 4, 5, 4, 1, 2); break;
    case 7: /* 11; 9,9,9; delta; 1 */ BC6H_MODE7(BC6H_GET) cfg = BC6HD_CFG(11, 9, 9, 9, 1, 1); break;
    case 10: /* 11; 4,4,5; delta; 2 */ BC6H_MODE10(BC6H_GET) part = bc6hd_bits(w, 77, 5); cfg = BC6HD_CFG(11, 4, 4, 5, 1, 2); break;
    case 11: /* 12; 8,8,8; delta; 1 */ BC6H_MODE11(BC6H_GET, BC6H_GET_REV) cfg = BC6HD_CFG(12, 8, 8, 8, 1, 1); break;
    case 14: /* 9; 5,5,5; delta; 2 */ BC6H_MODE14(BC6H_GET) part = bc6hd_bits(w, 77, 5); cfg = BC6HD_CFG(9, 5, 5, 5, 1, 2); break;
    case 15: /* 16; 4,4,4; delta; 1 */ BC6H_MODE15(BC6H_GET, BC6H_GET_REV) cfg = BC6HD_CFG(16, 4, 4, 4, 1, 1); break;
    case 18: /* 8; 6,5,5; delta; 2 */ BC6H_MODE18(BC6H_GET) part = bc6hd_bits(w, 77, 5); cfg = BC6HD_CFG(8, 6, 5, 5, 1, 2); break;
    case 22: /* 8; 5,6,5; delta; 2 */ BC6H_MODE22(BC6H_GET) part = bc6hd_bits(w, 77, 5); cfg = BC6HD_CFG(8, 5, 6, 5, 1, 2); break;
    case 26: /* 8; 5,5,6; delta; 2 */ BC6H_MODE26(BC6H_GET) part = bc6hd_bits(w, 77, 5); cfg = BC6HD_CFG(8, 5, 5, 6, 1, 2); break;
    case 30: /* 6; 6,6,6; plain; 2 */ BC6H_MODE30(BC6H_GET) part = bc6hd_bits(w, 77, 5); cfg = BC6HD_CFG(6, 6, 6, 6, 0, 2); break;
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
    for (int i = 0; i < 12; ++i) b->u[i] = regions ? bc6h_unq(e[i], epb) : 0u;
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
