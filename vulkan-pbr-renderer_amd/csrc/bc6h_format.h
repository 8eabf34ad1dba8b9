// bc6h_format.h -- what the BC6H_UF16 format fixes, written once for both directions: the encoders (bc6h_core.h, bc6h2_core.h) and the
// decoder (bc6h_decode_core.h) include it, and neither includes the other.  Nothing of either search is here.  Plain C and integer
// arithmetic only, for the device kernels and for a host compiler (host/pbr_ddsout.c and host/pbr_ddsin.c are C11): no rounding or
// denormal mode of either machine can change a bit.  tests/bc6h_ref.py, bc6h2_ref.py and bc6h_decode_ref.py restate it in numpy.
//
// Half codes: a texel channel is an unsigned half 0 .. 0x7BFF.  fp32 -> fp16 is round-to-nearest-even written out below; negative
// values, -0 and NaN give 0, +Inf and everything that rounds above 65504 give 0x7BFF, half subnormals are kept.
// Endpoints live in the scaled 16-bit space s = (h * 64 + 30) / 31, stored as codes of the mode's width epb:
//     unquantise: x for epb >= 15, 0 for 0, 0xFFFF for all ones, else ((x << 16) + 0x8000) >> epb
//     weights: 4-bit indices {0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64}, 3-bit {0, 9, 18, 27, 37, 46, 55, 64}
//     palette entry ((a (64 - w) + b w + 32) >> 6) * 31 >> 6, a half code
// Two-region modes: 32 partitions (bit t of bc6hd_subsets: texel t, row-major, belongs to the second subset), whose anchor is texel
// 15, 2 or 8.
// Block bits: the field lists at the end name, per mode, where every endpoint bit sits in the little-endian 128-bit block.
// No array is indexed by a run-time value and every position and width is a constant where a list is expanded: on the device
// everything stays in registers.
#pragma once
#include <stdint.h>
#if !defined(__cplusplus)
#include <stdbool.h>
#endif

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BC6H_FN __host__ __device__ __forceinline__
#define BC6H_UNROLL _Pragma("unroll")
#define BC6H_NO_UNROLL _Pragma("unroll 1")
#else
#define BC6H_FN static inline
#define BC6H_UNROLL
#define BC6H_NO_UNROLL
#endif

// fp32 bits -> fp16 bits, round to nearest even, sign, Inf and NaN kept (NaN becomes a quiet NaN): what the RGBA16F writer stores
BC6H_FN uint32_t bc6h_f16_from_f32(uint32_t bits) {
    const uint32_t sign = (bits >> 16) & 0x8000u, a = bits & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return sign | 0x7E00u;
    if (a >= 0x47800000u) return sign | 0x7C00u;                              // 65536 and above, Inf included
    const uint32_t e = a >> 23;
    if (e >= 113u) {                                                          // a normal half: drop 13 mantissa bits
        uint32_t h = (a - (112u << 23)) >> 13;
        const uint32_t rem = a & 0x1FFFu;
        h += (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ? 1u : 0u;      // may carry into the exponent, up to 0x7C00 = Inf
        return sign | h;
    }
    if (e < 102u) return sign;                                                // below half of the smallest half subnormal (fp32 subnormals too)
    const uint32_t mant = (a & 0x7FFFFFu) | 0x800000u, shift = 126u - e;      // 14 .. 24: units of 2^-24
    uint32_t h = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    h += (rem > half || (rem == half && (h & 1u))) ? 1u : 0u;
    return sign | h;
}
// fp16 bits -> the unsigned half code 0 .. 0x7BFF the encoder works on
BC6H_FN uint32_t bc6h_code_from_f16(uint32_t h) {
    if (h & 0x8000u) return 0u;                                               // negative, -0, -Inf, NaN with the sign set
    if (h > 0x7C00u) return 0u;                                               // NaN
    return h == 0x7C00u ? 0x7BFFu : h;
}
BC6H_FN uint32_t bc6h_code_from_f32(uint32_t bits) { return bc6h_code_from_f16(bc6h_f16_from_f32(bits)); }
// half code 0 .. 0x7BFF -> the fp32 bits of the same value: the exact widening, subnormal halves included, in integers
BC6H_FN uint32_t bc6hd_f32_from_code(uint32_t h) {
    if (h >= 0x400u) return (h << 13) + (112u << 23);
    if (h == 0u) return 0u;
    const uint32_t p = 31u - (uint32_t)__builtin_clz(h);                      // h 2^-24 = 1.m x 2^(p - 24), p = 0 .. 9
    return ((p + 103u) << 23) | ((h << (23u - p)) & 0x7FFFFFu);
}

BC6H_FN uint32_t bc6h_scale(uint32_t h) { return (h * 64u + 30u) / 31u; }     // half code -> the 16-bit space the endpoints live in
BC6H_FN uint32_t bc6h_unq(uint32_t x, uint32_t epb) {
    if (epb >= 15u) return x;
    if (x == 0u) return 0u;
    if (x == (1u << epb) - 1u) return 0xFFFFu;
    return ((x << 16) + 0x8000u) >> epb;
}
// the x in 0 .. 2^epb - 1 whose bc6h_unq(x, epb) is nearest to s (0 .. 65535), the lower x on a tie: one of s >> (16 - epb) and its
// two neighbours
BC6H_FN uint32_t bc6h_quantize(uint32_t s, uint32_t epb) {
    const uint32_t top = (1u << epb) - 1u, x1 = s >> (16u - epb), x0 = x1 > 0u ? x1 - 1u : 0u, x2 = x1 < top ? x1 + 1u : top;
    const int32_t d0 = (int32_t)bc6h_unq(x0, epb) - (int32_t)s, d1 = (int32_t)bc6h_unq(x1, epb) - (int32_t)s, d2 = (int32_t)bc6h_unq(x2, epb) - (int32_t)s;
    const uint32_t a0 = (uint32_t)(d0 < 0 ? -d0 : d0), a1 = (uint32_t)(d1 < 0 ? -d1 : d1), a2 = (uint32_t)(d2 < 0 ? -d2 : d2);
    uint32_t x = x0, best = a0;
    if (a1 < best) { best = a1; x = x1; }
    if (a2 < best) { x = x2; }
    return x;
}
BC6H_FN uint32_t bc6h_weight(uint32_t i) { return (i * 64u + 7u) / 15u; }     // {0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64}
BC6H_FN uint32_t bc6hd_weight3(uint32_t i) { return (i * 64u + 3u) / 7u; }    // {0, 9, 18, 27, 37, 46, 55, 64}
// palette entry of unquantised endpoints a, b at weight w, as a half code (at most 0x7BFF)
BC6H_FN uint32_t bc6h_palette(uint32_t a, uint32_t b, uint32_t w) { return (((a * (64u - w) + b * w + 32u) >> 6) * 31u) >> 6; }

BC6H_FN uint32_t bc6hd_subsets(uint32_t partition) {                          // bit t: texel t belongs to the second subset
    static const uint16_t k[32] = {0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
                                   0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C};
    return k[partition & 31u];
}
BC6H_FN uint32_t bc6hd_anchor(uint32_t partition) {                           // the second subset's anchor texel: 15, 2 or 8
    const uint64_t nibbles = (partition & 16u) ? 0x22882282F882282Full : 0xFFFFFFFFFFFFFFFFull;
    return (uint32_t)(nibbles >> (4u * (partition & 15u))) & 15u;
}

// bits pos .. pos + n - 1 of the block, n <= 31; pos and n are constants at every call, so the word index is one too
BC6H_FN uint32_t bc6hd_bits(const uint32_t w[4], uint32_t pos, uint32_t n) {
    const uint32_t i = pos >> 5, s = pos & 31u;
    uint32_t v = w[i] >> s;
    if (s + n > 32u) v |= w[i + 1u] << (32u - s);                             // pos + n <= 128: i + 1 <= 3 here
    return v & ((1u << n) - 1u);
}
// v's low n bits at block bits pos .. pos + n - 1; pos and n are constants at every call, and no field is written twice
BC6H_FN void bc6h_put_bits(uint32_t w[4], uint32_t pos, uint32_t n, uint32_t v) {
    const uint32_t i = pos >> 5, s = pos & 31u;
    v &= (1u << n) - 1u;
    w[i] |= v << s;
    if (s + n > 32u) w[i + 1u] |= v >> (32u - s);                             // pos + n <= 128: i + 1 <= 3 here
}
BC6H_FN uint32_t bc6hd_rev(uint32_t v, uint32_t n) {                          // the low n bits in reverse order
    uint32_t r = 0;
    BC6H_UNROLL
    for (uint32_t i = 0; i < 6u; ++i) if (i < n) r |= ((v >> i) & 1u) << (n - 1u - i);
    return r;
}

// The endpoint fields of the 14 modes, named by the mode field's value.  An entry F(slot, bit, pos, n): the n block bits from pos are
// bits bit .. bit + n - 1 of endpoint slot 3 E + c (endpoint E = 0 .. 3, channel c); R is the same with the bits in reverse order
// (modes 11 and 15 only).  A list is expanded with the entry macros below, where w[4] is the block and e[12] the endpoint fields as
// stored (deltas where the mode has them).  The mode field itself and, in the two-region modes, the partition at bits 77 .. 81 are
// not in the lists.
#define BC6H_GET(slot, bit, pos, n) e[slot] |= bc6hd_bits(w, pos, n) << (bit);
#define BC6H_GET_REV(slot, bit, pos, n) e[slot] |= bc6hd_rev(bc6hd_bits(w, pos, n), n) << (bit);
#define BC6H_PUT(slot, bit, pos, n) bc6h_put_bits(w, pos, n, e[slot] >> (bit));

#define BC6H_BASE10(F) F(0, 0, 5, 10) F(1, 0, 15, 10) F(2, 0, 25, 10)        /* bits 5 .. 34 of modes 2, 3, 6, 7, 10, 11 and 15 */
#define BC6H_TAIL5(F) /* bits 35 .. 76 of modes 0 and 14 */ \
    F(3, 0, 35, 5) F(10, 4, 40, 1) F(7, 0, 41, 4) F(4, 0, 45, 5) F(11, 0, 50, 1) F(10, 0, 51, 4) F(5, 0, 55, 5) F(11, 1, 60, 1) \
    F(8, 0, 61, 4) F(6, 0, 65, 5) F(11, 2, 70, 1) F(9, 0, 71, 5) F(11, 3, 76, 1)
#define BC6H_TAIL6(F) /* bits 35 .. 76 of modes 1 and 30 */ \
    F(3, 0, 35, 6) F(7, 0, 41, 4) F(4, 0, 45, 6) F(10, 0, 51, 4) F(5, 0, 55, 6) F(8, 0, 61, 4) F(6, 0, 65, 6) F(9, 0, 71, 6)

#define BC6H_MODE0(F) F(7, 4, 2, 1) F(8, 4, 3, 1) F(11, 4, 4, 1) F(0, 0, 5, 10) F(1, 0, 15, 10) F(2, 0, 25, 10) BC6H_TAIL5(F)
#define BC6H_MODE1(F) \
    F(7, 5, 2, 1) F(10, 4, 3, 1) F(10, 5, 4, 1) F(0, 0, 5, 7) F(11, 0, 12, 1) F(11, 1, 13, 1) F(8, 4, 14, 1) F(1, 0, 15, 7) \
    F(8, 5, 22, 1) F(11, 2, 23, 1) F(7, 4, 24, 1) F(2, 0, 25, 7) F(11, 3, 32, 1) F(11, 5, 33, 1) F(11, 4, 34, 1) BC6H_TAIL6(F)
#define BC6H_MODE2(F) \
    BC6H_BASE10(F) F(3, 0, 35, 5) F(0, 10, 40, 1) F(7, 0, 41, 4) F(4, 0, 45, 4) F(1, 10, 49, 1) F(11, 0, 50, 1) F(10, 0, 51, 4) \
    F(5, 0, 55, 4) F(2, 10, 59, 1) F(11, 1, 60, 1) F(8, 0, 61, 4) F(6, 0, 65, 5) F(11, 2, 70, 1) F(9, 0, 71, 5) F(11, 3, 76, 1)
#define BC6H_MODE3(F) BC6H_BASE10(F) F(3, 0, 35, 10) F(4, 0, 45, 10) F(5, 0, 55, 10)
#define BC6H_MODE6(F) \
    BC6H_BASE10(F) F(3, 0, 35, 4) F(0, 10, 39, 1) F(10, 4, 40, 1) F(7, 0, 41, 4) F(4, 0, 45, 5) F(1, 10, 50, 1) F(10, 0, 51, 4) \
    F(5, 0, 55, 4) F(2, 10, 59, 1) F(11, 1, 60, 1) F(8, 0, 61, 4) F(6, 0, 65, 4) F(11, 0, 69, 1) F(11, 2, 70, 1) F(9, 0, 71, 4) \
    F(7, 4, 75, 1) F(11, 3, 76, 1)
#define BC6H_MODE7(F) BC6H_BASE10(F) F(3, 0, 35, 9) F(0, 10, 44, 1) F(4, 0, 45, 9) F(1, 10, 54, 1) F(5, 0, 55, 9) F(2, 10, 64, 1)
#define BC6H_MODE10(F) \
    BC6H_BASE10(F) F(3, 0, 35, 4) F(0, 10, 39, 1) F(8, 4, 40, 1) F(7, 0, 41, 4) F(4, 0, 45, 4) F(1, 10, 49, 1) F(11, 0, 50, 1) \
    F(10, 0, 51, 4) F(5, 0, 55, 5) F(2, 10, 60, 1) F(8, 0, 61, 4) F(6, 0, 65, 4) F(11, 1, 69, 1) F(11, 2, 70, 1) F(9, 0, 71, 4) \
    F(11, 4, 75, 1) F(11, 3, 76, 1)
#define BC6H_MODE11(F, R) BC6H_BASE10(F) F(3, 0, 35, 8) R(0, 10, 43, 2) F(4, 0, 45, 8) R(1, 10, 53, 2) F(5, 0, 55, 8) R(2, 10, 63, 2)
#define BC6H_MODE14(F) F(0, 0, 5, 9) F(8, 4, 14, 1) F(1, 0, 15, 9) F(7, 4, 24, 1) F(2, 0, 25, 9) F(11, 4, 34, 1) BC6H_TAIL5(F)
#define BC6H_MODE15(F, R) BC6H_BASE10(F) F(3, 0, 35, 4) R(0, 10, 39, 6) F(4, 0, 45, 4) R(1, 10, 49, 6) F(5, 0, 55, 4) R(2, 10, 59, 6)
#define BC6H_MODE18(F) \
    F(0, 0, 5, 8) F(10, 4, 13, 1) F(8, 4, 14, 1) F(1, 0, 15, 8) F(11, 2, 23, 1) F(7, 4, 24, 1) F(2, 0, 25, 8) F(11, 3, 33, 1) \
    F(11, 4, 34, 1) F(3, 0, 35, 6) F(7, 0, 41, 4) F(4, 0, 45, 5) F(11, 0, 50, 1) F(10, 0, 51, 4) F(5, 0, 55, 5) F(11, 1, 60, 1) \
    F(8, 0, 61, 4) F(6, 0, 65, 6) F(9, 0, 71, 6)
#define BC6H_MODE22(F) \
    F(0, 0, 5, 8) F(11, 0, 13, 1) F(8, 4, 14, 1) F(1, 0, 15, 8) F(7, 5, 23, 1) F(7, 4, 24, 1) F(2, 0, 25, 8) F(10, 5, 33, 1) \
    F(11, 4, 34, 1) F(3, 0, 35, 5) F(10, 4, 40, 1) F(7, 0, 41, 4) F(4, 0, 45, 6) F(10, 0, 51, 4) F(5, 0, 55, 5) F(11, 1, 60, 1) \
    F(8, 0, 61, 4) F(6, 0, 65, 5) F(11, 2, 70, 1) F(9, 0, 71, 5) F(11, 3, 76, 1)
#define BC6H_MODE26(F) \
    F(0, 0, 5, 8) F(11, 1, 13, 1) F(8, 4, 14, 1) F(1, 0, 15, 8) F(8, 5, 23, 1) F(7, 4, 24, 1) F(2, 0, 25, 8) F(11, 5, 33, 1) \
    F(11, 4, 34, 1) F(3, 0, 35, 5) F(10, 4, 40, 1) F(7, 0, 41, 4) F(4, 0, 45, 5) F(11, 0, 50, 1) F(10, 0, 51, 4) F(5, 0, 55, 6) \
    F(8, 0, 61, 4) F(6, 0, 65, 5) F(11, 2, 70, 1) F(9, 0, 71, 5) F(11, 3, 76, 1)
#define BC6H_MODE30(F) \
    F(0, 0, 5, 6) F(10, 4, 11, 1) F(11, 0, 12, 1) F(11, 1, 13, 1) F(8, 4, 14, 1) F(1, 0, 15, 6) F(7, 5, 21, 1) F(8, 5, 22, 1) \
    F(11, 2, 23, 1) F(7, 4, 24, 1) F(2, 0, 25, 6) F(10, 5, 31, 1) F(11, 3, 32, 1) F(11, 5, 33, 1) F(11, 4, 34, 1) BC6H_TAIL6(F)
