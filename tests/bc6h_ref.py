"""The BC6H encode contract of csrc/bc6h_core.h (K18) restated in numpy, vectorised over blocks: the reference of the host build of the
header and of the kernel, byte for byte.  Integers only (int64); see the header for the rules.

encode / encode_bbox take one level [layers][h][w][4] as float32 (RGBA32F) or uint16 (the bits of RGBA16F) and return the blocks as
uint8 [layers * ceil(h/4) * ceil(w/4)][16], row-major within a layer, layer after layer.  decode handles mode 11 only."""
import numpy as np

WEIGHTS = np.array([0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64], np.int64)
MAX_CODE = 0x7BFF


def f16_from_f32(bits):
    """fp32 bits -> fp16 bits, round to nearest even, sign / Inf / NaN kept: the header's bc6h_f16_from_f32"""
    bits = np.asarray(bits).astype(np.int64)
    sign = (bits >> 16) & 0x8000
    a = bits & 0x7FFFFFFF
    e = a >> 23
    h = (a - (112 << 23)) >> 13
    rem = a & 0x1FFF
    normal = h + ((rem > 0x1000) | ((rem == 0x1000) & ((h & 1) == 1)))
    shift = np.clip(126 - e, 14, 24)
    mant = (a & 0x7FFFFF) | 0x800000
    hs = mant >> shift
    rs = mant & ((1 << shift) - 1)
    half = 1 << (shift - 1)
    sub = hs + ((rs > half) | ((rs == half) & ((hs & 1) == 1)))
    out = np.where(e >= 113, normal, np.where(e < 102, 0, sub))
    out = np.where(a >= 0x47800000, 0x7C00, out)
    out = np.where(a > 0x7F800000, 0x7E00, out)
    return sign | out


def code_from_f16(h):
    h = np.asarray(h).astype(np.int64)
    return np.where((h & 0x8000) != 0, 0, np.where(h > 0x7C00, 0, np.where(h == 0x7C00, MAX_CODE, h)))


def half_codes(level):
    """[..., 4] float32 or uint16 -> [..., 3] int64 half codes 0 .. 0x7BFF"""
    level = np.asarray(level)
    if level.dtype == np.float32:
        return code_from_f16(f16_from_f32(np.ascontiguousarray(level[..., :3]).view(np.uint32)))
    assert level.dtype == np.uint16, level.dtype
    return code_from_f16(level[..., :3])


def block_texels(codes):
    """[layers][h][w][3] -> [layers * bh * bw][16][3] with the clamped edge rule"""
    L, h, w, _ = codes.shape
    bh, bw = (h + 3) // 4, (w + 3) // 4
    ys = np.minimum(np.arange(bh * 4), h - 1)
    xs = np.minimum(np.arange(bw * 4), w - 1)
    p = codes[:, ys][:, :, xs]                                                # [L][4 bh][4 bw][3]
    p = p.reshape(L, bh, 4, bw, 4, 3).transpose(0, 1, 3, 2, 4, 5)
    return p.reshape(L * bh * bw, 16, 3)


def scale(h):
    return (h * 64 + 30) // 31


def unq(x):
    return np.where(x == 0, 0, np.where(x == 1023, 0xFFFF, ((x << 16) + 0x8000) >> 10))


def quantize(s):
    x1 = s >> 6
    cand = np.stack([np.maximum(x1 - 1, 0), x1, np.minimum(x1 + 1, 1023)])
    k = np.argmin(np.abs(unq(cand) - s[None]), axis=0)                        # the first minimum: the lowest x
    return np.take_along_axis(cand, k[None], axis=0)[0]


def palette(ua, ub):
    """[N][3] unquantised endpoints -> [N][16][3] half codes"""
    w = WEIGHTS[None, :, None]
    return (((ua[:, None, :] * (64 - w) + ub[:, None, :] * w + 32) >> 6) * 31) >> 6


def _try(h, ea, eb):
    qa, qb = quantize(ea), quantize(eb)
    pal = palette(unq(qa), unq(qb))
    best = idx = None
    for i in range(16):                                                       # entry by entry: a strict < keeps the lowest i
        err = ((pal[:, i, None, :] - h) ** 2).sum(axis=2)                     # [N][texel]
        if best is None:
            best, idx = err, np.zeros(err.shape, np.int64)
        else:
            better = err < best
            idx[better] = i
            best = np.minimum(best, err)
    return qa, qb, idx, best.sum(axis=1)


def candidates(h):
    """the three endpoint pairs of the contract, in scaled space: list of (ea, eb), each [N][3]"""
    s = scale(h)
    lo, hi = s.min(axis=1), s.max(axis=1)
    tot = s.sum(axis=1)
    flip = np.zeros(lo.shape, bool)
    for c in (1, 2):
        flip[:, c] = 16 * (s[:, :, 0] * s[:, :, c]).sum(axis=1) - tot[:, 0] * tot[:, c] < 0
    out = [(lo, hi), (np.where(flip, hi, lo), np.where(flip, lo, hi))]
    inset = (hi - lo) >> 4
    out.append((np.where(flip, hi - inset, lo + inset), np.where(flip, lo + inset, hi - inset)))
    return out


def encode_texels(h, ncand=3):
    """[N][16][3] half codes -> (endpoints [N][6], indices [N][16], squared error [N]) after the anchor rule"""
    best = None
    for ea, eb in candidates(h)[:ncand]:
        qa, qb, idx, err = _try(h, ea, eb)
        if best is None:
            best = [qa, qb, idx, err]
        else:
            better = err < best[3]                                            # strict: the earlier candidate wins a tie
            best = [np.where(better[:, None], qa, best[0]), np.where(better[:, None], qb, best[1]),
                    np.where(better[:, None], idx, best[2]), np.where(better, err, best[3])]
    qa, qb, idx, err = best
    swap = idx[:, 0] >= 8
    idx = np.where(swap[:, None], 15 - idx, idx)
    qa, qb = np.where(swap[:, None], qb, qa), np.where(swap[:, None], qa, qb)
    return np.concatenate([qa, qb], axis=1), idx, err


def pack(q, idx):
    ends = np.zeros(len(q), np.uint64)
    for k in range(6):
        ends |= q[:, k].astype(np.uint64) << np.uint64(10 * k)
    lo = np.uint64(3) | (ends << np.uint64(5))                                # the top bit of `ends` falls off: it is bit 64
    hi = (ends >> np.uint64(59)) | (idx[:, 0].astype(np.uint64) << np.uint64(1))
    for t in range(1, 16):
        hi |= idx[:, t].astype(np.uint64) << np.uint64(4 * t)
    return np.stack([lo, hi], axis=1).astype("<u8").view(np.uint8).reshape(-1, 16)


def _encode(level, ncand, chunk=8192):
    h = block_texels(half_codes(level))
    out, errs = [], []
    for i in range(0, len(h), chunk):
        q, idx, err = encode_texels(h[i:i + chunk], ncand)
        out.append(pack(q, idx))
        errs.append(err)
    return np.concatenate(out), np.concatenate(errs)


def encode(level):
    return _encode(level, 3)[0]


def encode_bbox(level):
    return _encode(level, 1)[0]


def decode(blocks):
    """uint8 [N][16] -> half codes int64 [N][16][3]; mode 11 only"""
    b = np.ascontiguousarray(np.asarray(blocks, np.uint8).reshape(-1, 16)).view("<u8").astype(np.uint64)
    lo, hi = b[:, 0], b[:, 1]
    if ((lo & np.uint64(31)) != 3).any():
        raise ValueError("decode handles BC6H mode 11 (mode bits 00011) only")
    ends = (lo >> np.uint64(5)) | ((hi & np.uint64(1)) << np.uint64(59))
    q = np.stack([(ends >> np.uint64(10 * k)) & np.uint64(1023) for k in range(6)], axis=1).astype(np.int64)
    idx = np.stack([(hi >> np.uint64(1)) & np.uint64(7)] + [(hi >> np.uint64(4 * t)) & np.uint64(15) for t in range(1, 16)], axis=1).astype(np.int64)
    pal = palette(unq(q[:, :3]), unq(q[:, 3:]))
    return np.take_along_axis(pal, idx[:, :, None], axis=1)


def winning_candidate(level):
    """per block: which of the three candidates the contract keeps (0, 1, 2)"""
    h = block_texels(half_codes(level))
    errs = np.stack([_try(h, ea, eb)[3] for ea, eb in candidates(h)])
    return np.argmin(errs, axis=0)                                            # the first minimum: the earlier candidate


def decode_level(blocks, w, h, layers):
    """blocks of one level -> float32 [layers][h][w][3]"""
    bh, bw = (h + 3) // 4, (w + 3) // 4
    codes = decode(blocks).reshape(layers, bh, bw, 4, 4, 3).transpose(0, 1, 3, 2, 4, 5).reshape(layers, bh * 4, bw * 4, 3)
    return codes[:, :h, :w].astype(np.uint16).view(np.float16).astype(np.float32)


def level_bytes(w, h, layers):
    return ((w + 3) // 4) * ((h + 3) // 4) * 16 * layers


# ---- the shapes of the tests ----
def hdr_level(w, h, layers, seed):
    """smooth HDR content with a warm-to-cold gradient, grain and a few texels far above 1"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = (x + 0.5) / w, (y + 0.5) / h
    out = np.empty((layers, h, w, 4), np.float64)
    for l in range(layers):
        base = 0.05 + 3.0 * np.exp(-6.0 * ((u - 0.3 - 0.1 * l) ** 2 + (v - 0.6) ** 2))
        out[l, ..., 0] = base * (0.4 + 1.2 * v)
        out[l, ..., 1] = base * 0.8
        out[l, ..., 2] = base * (1.6 - 1.2 * v)                               # blue falls as red rises
        out[l, ..., 3] = 1.0
    out[..., :3] *= np.exp(0.15 * rng.standard_normal(out[..., :3].shape))
    hot = rng.random((layers, h, w)) < 0.01
    out[hot, :3] *= 2000.0
    return out.astype(np.float32)


# a block of noisy HDR content on which candidate 3 has the lowest error (every value is exact in fp16)
INSET_BLOCK = [[3.0234375, 2.080078125, 2.6875], [3.3671875, 3.302734375, 3.271484375], [3.89453125, 2.322265625, 2.525390625],
               [3.009765625, 1.9931640625, 2.42578125], [2.9765625, 2.99609375, 2.451171875], [3.060546875, 2.453125, 2.630859375],
               [3.568359375, 2.740234375, 2.0234375], [3.44921875, 2.37109375, 2.658203125], [3.00390625, 2.0703125, 2.345703125],
               [4.34765625, 2.1015625, 3.017578125], [3.40625, 2.328125, 3.298828125], [2.0859375, 2.12109375, 2.21484375],
               [3.095703125, 2.083984375, 2.384765625], [3.642578125, 2.5546875, 2.166015625], [3.26171875, 2.03125, 2.27734375],
               [3.39453125, 2.33203125, 1.81640625]]


def hostile_blocks():
    """one row of crafted 4 x 4 blocks, float32 [1][4][4 k][4]; every rule of the conversion and every candidate path"""
    f = np.float32
    sub32 = np.array([1, 0x7FFFFF, 0x80000001], np.uint32).view(f)                # fp32 subnormals, one negative
    blocks = []

    def add(rgb16):
        b = np.ones((4, 4, 4), f)
        b[..., :3] = np.asarray(rgb16, f).reshape(4, 4, 3)
        blocks.append(b)

    specials = [-1.0, -0.0, np.nan, np.inf, -np.inf, 1e30, 65504.0, 65520.0, 65519.99, 6e-8, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 8.9e-8, 6.1e-5, 6.0975552e-5, 1.0]
    add([[s, 0.5, 2.0] for s in specials])
    add([[0.25, s, 1e-3] for s in specials])
    add([[sub32[i % 3], 3e-8 * (i + 1), 5.96e-8 * i] for i in range(16)])       # fp32 subnormals next to half subnormals
    add([[0.7, 0.7, 0.7]] * 16)                                                   # all equal
    add([[0.0, 0.0, 0.0]] * 16)                                                   # all zero
    add([[4.0 - 0.2 * i] * 3 for i in range(16)])                                 # texel 0 the brightest: the swap path
    add([[0.1 + 0.1 * i, 0.5, 1.7 - 0.1 * i] for i in range(16)])                 # red rises as blue falls: candidate 2
    add([[0.1 + 0.1 * i, 1.7 - 0.1 * i, 1.7 - 0.1 * i] for i in range(16)])       # both flipped
    add(INSET_BLOCK)                                                              # noisy texels with outliers: the inset wins
    add([[65504.0, 1e-7 * i, 70000.0] for i in range(16)])
    return np.concatenate(blocks, axis=1)[None]


def as_half_bits(level32):
    """the RGBA16F twin of a float32 level: numpy's conversion (the same round-to-nearest-even), as uint16 bits"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(level32, np.float32).astype(np.float16).view(np.uint16)


def hostile_blocks_f16():
    """the hostile row as RGBA16F bits, plus patterns only half bits can carry: negative NaN, subnormals, -Inf"""
    bits = as_half_bits(hostile_blocks())
    extra = np.zeros((1, 4, 4, 4), np.uint16)
    pats = [0x0001, 0x03FF, 0x0400, 0x7BFF, 0x7C00, 0x7C01, 0x7E00, 0xFE00, 0xFC00, 0x8000, 0x8001, 0xBC00, 0x3C00, 0x0200, 0x7FFF, 0xFFFF]
    extra[0, :, :, 0] = np.array(pats, np.uint16).reshape(4, 4)
    extra[0, :, :, 1] = np.array(pats[::-1], np.uint16).reshape(4, 4)
    extra[0, :, :, 2] = 0x3800
    extra[0, :, :, 3] = 0x3C00
    return np.concatenate([bits, extra], axis=2)


CUBE_FACES = (1, 2, 3, 4, 5, 6, 12, 20, 68, 260)
FLAT_LEVELS = ((7, 9), (20, 12))


def cases():
    """(name, level) with level float32 or uint16 [layers][h][w][4]: every shape of the issue in both source formats"""
    out = []
    for n in CUBE_FACES:
        lvl = hdr_level(n, n, 6, 100 + n)
        out.append((f"cube{n}_f32", lvl))
        out.append((f"cube{n}_f16", as_half_bits(lvl)))
    for w, h in FLAT_LEVELS:
        lvl = hdr_level(w, h, 1, 1000 * w + h)
        out.append((f"flat{w}x{h}_f32", lvl))
        out.append((f"flat{w}x{h}_f16", as_half_bits(lvl)))
    out.append(("hostile_f32", hostile_blocks()))
    out.append(("hostile_f16", hostile_blocks_f16()))
    return out
