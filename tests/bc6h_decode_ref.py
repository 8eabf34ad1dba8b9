"""The BC6H_UF16 decode contract (K19) restated in numpy from the format's tables, vectorised over blocks: the reference of the host
build of csrc/bc6h_decode_core.h, of PBR_DecodeBC6HBlocks and of the kernel, byte for byte.  Integers only (int64).

A block of 16 bytes -> 16 texels x 3 half bit patterns in 0 .. 0x7BFF, row-major in the 4 x 4 block.  The low 2 bits are the mode if
they are 0 or 1, otherwise the low 5 bits; 19, 23, 27 and 31 are reserved and decode to zeros.  MODES holds, per mode value: endpoint
bits, delta bits (r, g, b), transformed, regions and the fields, read upward from the first bit after the mode bits:
    cE:n    n bits into the low bits of channel c of endpoint E (0 the base, then 1, 2, 3)
    cE:<k   one bit into bit k
    cE:n@kr n bits, bit-reversed, into bits k .. k + n - 1
Two-region modes end with a 5-bit partition.  Index bits start at 65 (one region: texel 0 has 3 bits, the others 4) or 82 (two
regions: texel 0 and the second subset's anchor have 2 bits, the others 3); exactly 128 bits are consumed."""
import numpy as np

MAX_CODE = 0x7BFF
RESERVED = (19, 23, 27, 31)

MODES = {
    0: (10, (5, 5, 5), True, 2, "g2:<4 b2:<4 b3:<4 r0:10 g0:10 b0:10 r1:5 g3:<4 g2:4 g1:5 b3:<0 g3:4 b1:5 b3:<1 b2:4 r2:5 b3:<2 r3:5 b3:<3"),
    1: (7, (6, 6, 6), True, 2, "g2:<5 g3:<4 g3:<5 r0:7 b3:<0 b3:<1 b2:<4 g0:7 b2:<5 b3:<2 g2:<4 b0:7 b3:<3 b3:<5 b3:<4 r1:6 g2:4 g1:6 g3:4 b1:6 b2:4 r2:6 r3:6"),
    2: (11, (5, 4, 4), True, 2, "r0:10 g0:10 b0:10 r1:5 r0:<10 g2:4 g1:4 g0:<10 b3:<0 g3:4 b1:4 b0:<10 b3:<1 b2:4 r2:5 b3:<2 r3:5 b3:<3"),
    6: (11, (4, 5, 4), True, 2, "r0:10 g0:10 b0:10 r1:4 r0:<10 g3:<4 g2:4 g1:5 g0:<10 g3:4 b1:4 b0:<10 b3:<1 b2:4 r2:4 b3:<0 b3:<2 r3:4 g2:<4 b3:<3"),
    10: (11, (4, 4, 5), True, 2, "r0:10 g0:10 b0:10 r1:4 r0:<10 b2:<4 g2:4 g1:4 g0:<10 b3:<0 g3:4 b1:5 b0:<10 b2:4 r2:4 b3:<1 b3:<2 r3:4 b3:<4 b3:<3"),
    14: (9, (5, 5, 5), True, 2, "r0:9 b2:<4 g0:9 g2:<4 b0:9 b3:<4 r1:5 g3:<4 g2:4 g1:5 b3:<0 g3:4 b1:5 b3:<1 b2:4 r2:5 b3:<2 r3:5 b3:<3"),
    18: (8, (6, 5, 5), True, 2, "r0:8 g3:<4 b2:<4 g0:8 b3:<2 g2:<4 b0:8 b3:<3 b3:<4 r1:6 g2:4 g1:5 b3:<0 g3:4 b1:5 b3:<1 b2:4 r2:6 r3:6"),
    22: (8, (5, 6, 5), True, 2, "r0:8 b3:<0 b2:<4 g0:8 g2:<5 g2:<4 b0:8 g3:<5 b3:<4 r1:5 g3:<4 g2:4 g1:6 g3:4 b1:5 b3:<1 b2:4 r2:5 b3:<2 r3:5 b3:<3"),
    26: (8, (5, 5, 6), True, 2, "r0:8 b3:<1 b2:<4 g0:8 b2:<5 g2:<4 b0:8 b3:<5 b3:<4 r1:5 g3:<4 g2:4 g1:5 b3:<0 g3:4 b1:6 b2:4 r2:5 b3:<2 r3:5 b3:<3"),
    30: (6, (6, 6, 6), False, 2, "r0:6 g3:<4 b3:<0 b3:<1 b2:<4 g0:6 g2:<5 b2:<5 b3:<2 g2:<4 b0:6 g3:<5 b3:<3 b3:<5 b3:<4 r1:6 g2:4 g1:6 g3:4 b1:6 b2:4 r2:6 r3:6"),
    3: (10, (10, 10, 10), False, 1, "r0:10 g0:10 b0:10 r1:10 g1:10 b1:10"),
    7: (11, (9, 9, 9), True, 1, "r0:10 g0:10 b0:10 r1:9 r0:<10 g1:9 g0:<10 b1:9 b0:<10"),
    11: (12, (8, 8, 8), True, 1, "r0:10 g0:10 b0:10 r1:8 r0:2@10r g1:8 g0:2@10r b1:8 b0:2@10r"),
    15: (16, (4, 4, 4), True, 1, "r0:10 g0:10 b0:10 r1:4 r0:6@10r g1:4 g0:6@10r b1:4 b0:6@10r"),
}
MODE_VALUES = tuple(sorted(list(MODES) + list(RESERVED)))                     # the 18 values the mode bits can take

# texel 0 first, 1 = second subset
PARTITIONS = """
0011001100110011 0001000100010001 0111011101110111 0001001100110111 0000000100010011 0011011101111111 0001001101111111 0000000100110111
0000000000010011 0011011111111111 0000000101111111 0000000000010111 0001011111111111 0000000011111111 0000111111111111 0000000000001111
0000100011101111 0111000100000000 0000000010001110 0111001100010000 0011000100000000 0000100011001110 0000000010001100 0111001100110001
0011000100010000 0000100010001100 0110011001100110 0011011001101100 0001011111101000 0000111111110000 0111000110001110 0011100110011100
""".split()
SUBSET = np.array([[int(c) for c in p] for p in PARTITIONS], np.int64)        # [partition][texel]
ANCHOR = np.array([15] * 17 + [2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2], np.int64)
WEIGHTS3 = np.array([0, 9, 18, 27, 37, 46, 55, 64], np.int64)
WEIGHTS4 = np.array([0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64], np.int64)


def parse_fields(text):
    """-> list of (channel 0..2, endpoint 0..3, bits read, destination bit, reversed)"""
    out = []
    for f in text.split():
        name, spec = f.split(":")
        c, e = "rgb".index(name[0]), int(name[1])
        if spec.startswith("<"):
            out.append((c, e, 1, int(spec[1:]), False))
        elif "@" in spec:
            n, k = spec.split("@")
            assert k.endswith("r")
            out.append((c, e, int(n), int(k[:-1]), True))
        else:
            out.append((c, e, int(spec), 0, False))
    return out


def modes_of(blocks):
    b0 = np.asarray(blocks, np.uint8).reshape(-1, 16)[:, 0].astype(np.int64)
    return np.where((b0 & 3) < 2, b0 & 3, b0 & 31)


def _take(bits, pos, n):
    """bits [N][128] (bit 0 first), pos scalar or [N] -> the n-bit field at pos as int64 [N]"""
    pos = np.broadcast_to(np.asarray(pos, np.int64), (len(bits),))
    v = np.zeros(len(bits), np.int64)
    for i in range(n):
        v |= np.take_along_axis(bits, (pos + i)[:, None], axis=1)[:, 0] << i
    return v


def unquantize(x, epb):
    if epb >= 15:
        return x
    return np.where(x == 0, 0, np.where(x == (1 << epb) - 1, 0xFFFF, ((x << 15) + 0x4000) >> (epb - 1)))


def _decode_mode(bits, mode):
    epb, delta, transformed, regions, text = MODES[mode]
    n = len(bits)
    e = np.zeros((n, 4, 3), np.int64)
    pos = 2 if mode < 2 else 5
    for c, k, cnt, dst, rev in parse_fields(text):
        v = _take(bits, pos, cnt)
        if rev:
            v = sum(((v >> i) & 1) << (cnt - 1 - i) for i in range(cnt))
        e[:, k, c] |= v << dst
        pos += cnt
    part = np.zeros(n, np.int64)
    if regions == 2:
        part = _take(bits, pos, 5)
        pos += 5
    assert pos == (82 if regions == 2 else 65), (mode, pos)
    if transformed:
        for k in range(1, 2 * regions):
            for c in range(3):
                d = e[:, k, c]
                d = d - ((d >> (delta[c] - 1)) << delta[c])                   # sign extension from the channel's delta width
                e[:, k, c] = (e[:, 0, c] + d) & ((1 << epb) - 1)
    u = unquantize(e, epb)
    out = np.zeros((n, 16, 3), np.int64)
    anchor = ANCHOR[part]
    for t in range(16):
        if regions == 1:
            width = 3 if t == 0 else 4
            idx = _take(bits, pos, width)
            pos += width
            w = WEIGHTS4[idx]
            s = np.zeros(n, np.int64)
        else:
            width = np.where((t == 0) | (anchor == t), 2, 3)
            idx = np.where(width == 2, _take(bits, pos, 2), _take(bits, np.minimum(pos, 125), 3))
            pos = pos + width
            w = WEIGHTS3[idx]
            s = SUBSET[part, t]
        a = np.take_along_axis(u, (2 * s)[:, None, None].repeat(3, axis=2), axis=1)[:, 0]
        b = np.take_along_axis(u, (2 * s + 1)[:, None, None].repeat(3, axis=2), axis=1)[:, 0]
        out[:, t] = (((a * (64 - w[:, None]) + b * w[:, None] + 32) >> 6) * 31) >> 6
    assert np.all(pos == 128), mode
    return out


def decode(blocks):
    """uint8 [N][16] -> half codes int64 [N][16][3], every mode; reserved modes give zeros"""
    blocks = np.ascontiguousarray(np.asarray(blocks, np.uint8).reshape(-1, 16))
    bits = np.unpackbits(blocks, axis=1, bitorder="little").astype(np.int64)
    modes = modes_of(blocks)
    out = np.zeros((len(blocks), 16, 3), np.int64)
    for mode in MODES:
        sel = np.flatnonzero(modes == mode)
        if len(sel):
            out[sel] = _decode_mode(bits[sel], mode)
    return out


def decode_level_codes(blocks, w, h, layers):
    """blocks of one level, layer after layer -> half codes uint16 [layers][h][w][3]; texels of a block outside the level are dropped"""
    bh, bw = (h + 3) // 4, (w + 3) // 4
    codes = decode(blocks).reshape(layers, bh, bw, 4, 4, 3).transpose(0, 1, 3, 2, 4, 5).reshape(layers, bh * 4, bw * 4, 3)
    return np.ascontiguousarray(codes[:, :h, :w]).astype(np.uint16)


def level_rgba(blocks, w, h, layers, f32):
    """what the kernel writes: RGBA32F as float32 [layers][h][w][4] (the exact widening) or RGBA16F as uint16 bits; alpha 1.0"""
    codes = decode_level_codes(blocks, w, h, layers)
    out = np.empty(codes.shape[:3] + (4,), np.uint16)
    out[..., :3] = codes
    out[..., 3] = 0x3C00
    return out.view(np.float16).astype(np.float32) if f32 else out


def random_blocks(n, seed, mode=None):
    """n random blocks; `mode`: one of MODE_VALUES forced into the mode bits of every block, None: a random one of the 18 per block"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    m = np.full(n, mode, np.int64) if mode is not None else np.array(MODE_VALUES, np.int64)[rng.integers(0, len(MODE_VALUES), n)]
    two = m < 2
    b[:, 0] = np.where(two, (b[:, 0] & 0xFC) | m, (b[:, 0] & 0xE0) | m).astype(np.uint8)
    return b
