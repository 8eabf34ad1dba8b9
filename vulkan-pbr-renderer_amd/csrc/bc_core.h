// bc_core.h -- the block-compression decode contract (K15), written once for the device kernel of k_bc.hip and for a host
// compiler: integer arithmetic only.  Endpoints are widened by bit replication, interpolants use TRUNCATING division.
//   BC1 colour, c0 > c1 (always for the colour half of BC3): c0, c1, (2 c0 + c1) / 3, (c0 + 2 c1) / 3, alpha 255
//   BC1 colour, c0 <= c1: c0, c1, (c0 + c1) / 2, and index 3 = (0, 0, 0, 0) for BC1_RGBA_UN, (0, 0, 0, 255) for BC1_RGB_UN
//   BC3 alpha / BC5 channel, a0 > a1: a0, a1, ((7 - i) a0 + i a1) / 7 for i = 1 .. 6
//   BC3 alpha / BC5 channel, a0 <= a1: a0, a1, ((5 - i) a0 + i a1) / 5 for i = 1 .. 4, then 0, then 255
//   BC5 texel: (R, G, 0, 255), what geometry_pass.glsl:277-279 reads
// A block is passed as its little-endian 32-bit words (2 for BC1, 4 for BC3 / BC5); a texel comes back as r | g << 8 | b << 16 | a << 24,
// which is the RGBA8UN byte order on a little-endian machine (the device, and every host this is built for).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BC_FN __host__ __device__ __forceinline__
#else
#define BC_FN static inline
#endif

enum { BC_FMT_BC1_RGB = 0, BC_FMT_BC1_RGBA = 1, BC_FMT_BC3 = 2, BC_FMT_BC5 = 3 };

BC_FN uint32_t bc_block_bytes(int fmt) { return fmt == BC_FMT_BC1_RGB || fmt == BC_FMT_BC1_RGBA ? 8u : 16u; }

// 5:6:5 -> r | g << 8 | b << 16 with replicated low bits
BC_FN uint32_t bc_565(uint32_t c) {
    const uint32_t r5 = (c >> 11) & 31u, g6 = (c >> 5) & 63u, b5 = c & 31u;
    return ((r5 << 3) | (r5 >> 2)) | (((g6 << 2) | (g6 >> 4)) << 8) | (((b5 << 3) | (b5 >> 2)) << 16);
}
// (wa * a + wb * b) / div on each of the three colour bytes
BC_FN uint32_t bc_mix3(uint32_t a, uint32_t b, uint32_t wa, uint32_t wb, uint32_t div) {
    uint32_t o = 0;
    for (int s = 0; s < 24; s += 8) o |= ((wa * ((a >> s) & 255u) + wb * ((b >> s) & 255u)) / div) << s;
    return o;
}
// the four colours of a BC1 colour block (word0 = c0 | c1 << 16); four_only: the colour half of BC3; punch: index 3 of the 3-colour
// mode is transparent black (BC1_RGBA_UN) instead of opaque black
BC_FN void bc_color_palette(uint32_t word0, bool four_only, bool punch, uint32_t pal[4]) {
    const uint32_t c0 = word0 & 0xFFFFu, c1 = word0 >> 16;
    const uint32_t a = bc_565(c0), b = bc_565(c1), opaque = 0xFF000000u;
    pal[0] = a | opaque; pal[1] = b | opaque;
    if (c0 > c1 || four_only) { pal[2] = bc_mix3(a, b, 2, 1, 3) | opaque; pal[3] = bc_mix3(a, b, 1, 2, 3) | opaque; }
    else { pal[2] = bc_mix3(a, b, 1, 1, 2) | opaque; pal[3] = punch ? 0u : opaque; }
}
// pal[i] without a run-time indexed array (stays in registers on the device)
BC_FN uint32_t bc_pick(const uint32_t pal[4], uint32_t i) {
    const uint32_t lo = (i & 1u) ? pal[1] : pal[0], hi = (i & 1u) ? pal[3] : pal[2];
    return (i & 2u) ? hi : lo;
}
// value `idx` (0 .. 7) of an alpha / channel block with endpoints a0, a1
BC_FN uint32_t bc_alpha_value(uint32_t a0, uint32_t a1, uint32_t idx) {
    if (idx == 0) return a0;
    if (idx == 1) return a1;
    if (a0 > a1) return ((8u - idx) * a0 + (idx - 1u) * a1) / 7u;
    if (idx == 6) return 0u;
    if (idx == 7) return 255u;
    return ((6u - idx) * a0 + (idx - 1u) * a1) / 5u;
}
// the four values of row `row` of an alpha / channel block (two words: a0, a1, then 16 three-bit indices)
BC_FN void bc_alpha_row(uint32_t w0, uint32_t w1, int row, uint32_t out[4]) {
    const uint64_t bits = ((uint64_t)w1 << 16) | (w0 >> 16);                  // the 48 index bits
    const uint32_t r12 = (uint32_t)(bits >> (12 * row)) & 0xFFFu;
    const uint32_t a0 = w0 & 255u, a1 = (w0 >> 8) & 255u;
    for (int x = 0; x < 4; ++x) out[x] = bc_alpha_value(a0, a1, (r12 >> (3 * x)) & 7u);
}
// texels (0 .. 3, row) of one block
BC_FN void bc_decode_row(int fmt, const uint32_t* words, int row, uint32_t out[4]) {
    if (fmt == BC_FMT_BC5) {
        uint32_t r[4], g[4];
        bc_alpha_row(words[0], words[1], row, r);
        bc_alpha_row(words[2], words[3], row, g);
        for (int x = 0; x < 4; ++x) out[x] = r[x] | (g[x] << 8) | 0xFF000000u;
        return;
    }
    const bool bc3 = fmt == BC_FMT_BC3;
    const uint32_t* cw = bc3 ? words + 2 : words;
    uint32_t pal[4];
    bc_color_palette(cw[0], bc3, fmt == BC_FMT_BC1_RGBA, pal);
    const uint32_t idx = (cw[1] >> (8 * row)) & 255u;
    for (int x = 0; x < 4; ++x) out[x] = bc_pick(pal, (idx >> (2 * x)) & 3u);
    if (bc3) {
        uint32_t a[4];
        bc_alpha_row(words[0], words[1], row, a);
        for (int x = 0; x < 4; ++x) out[x] = (out[x] & 0x00FFFFFFu) | (a[x] << 24);
    }
}
