"""The two-region BC6H encode contract of csrc/bc6h2_core.h (K18, quality 1) restated in numpy, vectorised over blocks: the reference of
the host build of the header and of the kernel, byte for byte.  Integers only (int64); see the header for the rules.  The one-region
part is bc6h_ref's; the partition table, the anchors, the 3-bit weights and the field lists the packer walks are bc6h_decode_ref's,
which states them in another form than the header does.

encode2 takes one level [layers][h][w][4] as float32 (RGBA32F) or uint16 (the bits of RGBA16F) and returns the blocks as uint8
[layers * ceil(h/4) * ceil(w/4)][16]; encode2_texels takes half codes [N][16][3] and says what was chosen per block."""
import numpy as np

import bc6h_decode_ref as D
import bc6h_ref as R

CASES = (0, 14, 1, 30)                                                        # kind 1 .. 4; kind 0 is the one-region block
EPB = (10, 9, 7, 6)
DELTA = (5, 5, 6, 0)
LIMIT = (15, 15, 31)
ONE_REGION = 0


def quantize(s, epb):
    top = (1 << epb) - 1
    x1 = s >> (16 - epb)
    cand = np.stack([np.maximum(x1 - 1, 0), x1, np.minimum(x1 + 1, top)])
    k = np.argmin(np.abs(D.unquantize(cand, epb) - s[None]), axis=0)           # the first minimum: the lowest x
    return np.take_along_axis(cand, k[None], axis=0)[0]


def subset_endpoints(h):
    """[N][n][3] half codes of one subset -> (a, b) [N][3] in the scaled space: the box, G / B reversed on a negative covariance with R"""
    s = R.scale(h)
    n = s.shape[1]
    lo, hi, tot = s.min(axis=1), s.max(axis=1), s.sum(axis=1)
    flip = np.zeros(lo.shape, bool)
    for c in (1, 2):
        flip[:, c] = n * (s[:, :, 0] * s[:, :, c]).sum(axis=1) - tot[:, 0] * tot[:, c] < 0
    return np.where(flip, hi, lo), np.where(flip, lo, hi)


def try_partition(h, p):
    """steps 2 .. 4 for partition p -> (mode 0 .. 3 [N], quantised endpoints [N][4][3], indices [N][16], E2 [N])"""
    texels = [np.flatnonzero(D.SUBSET[p] == k) for k in (0, 1)]
    sp = np.stack(subset_endpoints(h[:, texels[0]]) + subset_endpoints(h[:, texels[1]]), axis=1)
    mode = np.full(len(h), 3, np.int64)
    q = quantize(sp, EPB[3])
    u = D.unquantize(q, EPB[3])
    for m in (2, 1, 0):                                                       # downwards: the first mode that fits is the last to overwrite
        qm = quantize(sp, EPB[m])
        fit = ((qm.max(axis=1) - qm.min(axis=1)) <= LIMIT[m]).all(axis=1)
        mode = np.where(fit, m, mode)
        q = np.where(fit[:, None, None], qm, q)
        u = np.where(fit[:, None, None], D.unquantize(qm, EPB[m]), u)
    idx = np.zeros((len(h), 16), np.int64)
    err = np.zeros(len(h), np.int64)
    w = D.WEIGHTS3[None, :, None]
    for k in (0, 1):
        pal = (((u[:, 2 * k, None, :] * (64 - w) + u[:, 2 * k + 1, None, :] * w + 32) >> 6) * 31) >> 6     # [N][8][3]
        e = ((pal[:, None, :, :] - h[:, texels[k]][:, :, None, :]) ** 2).sum(axis=3)                     # [N][texel][8]
        idx[:, texels[k]] = e.argmin(axis=2)                                  # the first minimum: the lowest i
        err += e.min(axis=2).sum(axis=1)
    return mode, q, idx, err


def search(h):
    """[N][16][3] half codes -> dict: kind, partition, err, and for the two-region blocks q [N][4][3], idx [N][16] after the anchor rule,
    swap0 / swap1 (whether a subset's endpoints were swapped); q1 / idx1 are the one-region block's"""
    n = len(h)
    q1, idx1, e1 = R.encode_texels(h)
    out = {"q1": q1, "idx1": idx1, "kind": np.zeros(n, np.int64), "partition": np.zeros(n, np.int64), "err": e1.copy(),
           "q": np.zeros((n, 4, 3), np.int64), "idx": np.zeros((n, 16), np.int64)}
    live = np.flatnonzero(e1 > 0)                                             # E1 = 0: nothing can be strictly better
    for p in range(32):
        if not len(live):
            break
        mode, q, idx, err = try_partition(h[live], p)
        better = err < out["err"][live]                                       # strict: the one-region block, then the lower p, wins a tie
        rows = live[better]
        out["kind"][rows], out["partition"][rows], out["err"][rows] = mode[better] + 1, p, err[better]
        out["q"][rows], out["idx"][rows] = q[better], idx[better]
    two = out["kind"] > 0
    sub = D.SUBSET[out["partition"]]                                          # [N][16]
    anchor = D.ANCHOR[out["partition"]]
    swap0 = two & (out["idx"][:, 0] >= 4)
    swap1 = two & (out["idx"][np.arange(n), anchor] >= 4)
    inv = np.where(sub == 1, swap1[:, None], swap0[:, None])
    out["idx"] = np.where(inv, 7 - out["idx"], out["idx"])
    q = out["q"].copy()
    q[swap0, 0], q[swap0, 1] = out["q"][swap0, 1], out["q"][swap0, 0]
    q[swap1, 2], q[swap1, 3] = out["q"][swap1, 3], out["q"][swap1, 2]
    out["q"], out["swap0"], out["swap1"] = q, swap0, swap1
    return out


def encode2_texels(h):
    """[N][16][3] half codes -> (kind [N]: 0 one region, 1 .. 4 = case 0 / 14 / 1 / 30; partition [N]; squared error [N])"""
    s = search(h)
    return s["kind"], s["partition"], s["err"]


def pack2(m, q, partition, idx):
    """blocks of one mode m: endpoints [n][4][3] and indices [n][16] after the anchor rule -> uint8 [n][16], by the decoder's field list"""
    case = CASES[m]
    epb, _, transformed, regions, text = D.MODES[case]
    assert epb == EPB[m] and regions == 2 and transformed == (DELTA[m] > 0)
    n = len(q)
    e = q.copy()
    if transformed:
        e[:, 1:] = (q[:, 1:] - q[:, :1]) & ((1 << DELTA[m]) - 1)
    bits = np.zeros((n, 128), np.uint8)
    pos = 2 if case < 2 else 5
    for i in range(pos):
        bits[:, i] = (case >> i) & 1
    for c, k, cnt, dst, rev in D.parse_fields(text):
        assert not rev
        for i in range(cnt):
            bits[:, pos + i] = (e[:, k, c] >> (dst + i)) & 1
        pos += cnt
    for i in range(5):
        bits[:, pos + i] = (partition >> i) & 1
    assert pos + 5 == 82
    at = np.full(n, 82, np.int64)
    anchor = D.ANCHOR[partition]
    for t in range(16):
        width = np.where((t == 0) | (anchor == t), 2, 3)
        assert (idx[:, t] < (1 << width)).all()                               # an anchor's index is below 4
        for i in range(3):
            rows = np.flatnonzero(i < width)
            bits[rows, at[rows] + i] = (idx[rows, t] >> i) & 1
        at = at + width
    assert (at == 128).all()
    return np.packbits(bits, axis=1, bitorder="little")


def encode2_blocks(h, chunk=4096):
    """[N][16][3] half codes -> (blocks uint8 [N][16], search dict of the whole input)"""
    blocks, parts = [], []
    for i in range(0, len(h), chunk):
        s = search(h[i:i + chunk])
        b = R.pack(s["q1"], s["idx1"])
        for m in range(4):
            rows = np.flatnonzero(s["kind"] == m + 1)
            if len(rows):
                b[rows] = pack2(m, s["q"][rows], s["partition"][rows], s["idx"][rows])
        blocks.append(b)
        parts.append(s)
    return np.concatenate(blocks), {k: np.concatenate([s[k] for s in parts]) for k in parts[0]}


def encode2(level):
    return encode2_blocks(R.block_texels(R.half_codes(level)))[0]


# ---- the shapes of the tests ----
def edge_scene(n=128, seed=0x5EED2E6E):
    """one RGBA32F layer [1][n][n][4] with hard edges: a sky gradient, dark ground behind a wavy horizon, a sun disc of 5e4 and a x30
    window, with 3 % grain"""
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    u, v = (x + 0.5) / n, (y + 0.5) / n
    sky = 0.3 + 2.0 * v
    rgb = np.stack([sky * (0.5 + v), sky * 0.8, sky * (1.6 - v)], axis=2)
    rgb[v > 0.62 + 0.05 * np.sin(9.0 * u)] *= 0.08
    rgb[(u - 0.3) ** 2 + (v - 0.25) ** 2 < 0.03 ** 2] = (5e4, 4.5e4, 3.5e4)
    rgb[(np.abs(u - 0.75) < 0.06) & (np.abs(v - 0.3) < 0.1)] *= 30.0
    rgb *= np.exp(0.03 * np.random.default_rng(seed).standard_normal(rgb.shape))
    out = np.ones((1, n, n, 4), np.float32)
    out[0, ..., :3] = rgb
    return out


def _level_of_blocks(blocks):
    """list of [16][3] half codes (texel order) -> RGBA16F bits [1][4][4 k][4], alpha 1.0"""
    out = np.full((1, 4, 4 * len(blocks), 4), 0x3C00, np.uint16)
    for i, b in enumerate(blocks):
        out[0, :, 4 * i:4 * i + 4, :3] = np.asarray(b, np.uint16).reshape(4, 4, 3)
    return out


def _split_block(p, codes0, codes1):
    """partition p's block: subset k's texels take codesk in texel order, cycled; an entry is one half code (grey) or three"""
    out = np.zeros((16, 3), np.int64)
    count = [0, 0]
    for t in range(16):
        k = int(D.SUBSET[p][t])
        src = (codes0, codes1)[k]
        out[t] = src[count[k] % len(src)]
        count[k] += 1
    return out


def half_of(value):
    return int(np.float16(value).view(np.uint16))


def as_float32(bits):
    """RGBA16F bits -> the RGBA32F level of the same values (every half is exact in fp32)"""
    return bits.view(np.float16).astype(np.float32)


def partition_strip():
    """RGBA16F bits [1][4][256][4], 64 blocks.  Block p < 32: two flat colours split by partition p's mask -- one region holds two
    colours as well as two regions do, so these tie and stay one-region.  Block 32 + p: the same split with a grey ramp in subset 0
    and a saturated red ramp in subset 1, which no single line holds: partition p wins."""
    flat = [_split_block(p, [[half_of(0.25), half_of(0.5), half_of(1.0)]], [[half_of(6.0), half_of(3.0), half_of(1.5)]]) for p in range(32)]
    ramp = [half_of(0.2 + 0.05 * i) for i in range(15)]
    hot = [[half_of(40.0 + 4.0 * i), half_of(2.0), half_of(0.01)] for i in range(15)]
    return _level_of_blocks(flat + [_split_block(p, ramp, hot) for p in range(32)])


# crafted blocks by name, in strip order; q10 / q7: the half code that quantises to x at 10 resp. 7 bits and decodes to itself
def q10(x):
    return 31 * x + 15


def q7(x):
    return 248 * x + 124


def spread_block(code, x0, x1, x2, x3, g):
    """partition 13 with R = B = code(x0), code(x1) in subset 0 and code(x2), code(x3) in subset 1 (x0 the least, x3 the greatest: the
    quantised spread is x3 - x0), G = code(g) resp. code(x0): the four colours are on no common line, so one region cannot hold them"""
    return _split_block(13, [[code(x0), code(g), code(x0)], [code(x1), code(g), code(x1)]], [[code(x2), code(x0), code(x2)], [code(x3), code(x0), code(x3)]])


def crafted_blocks():
    up = [half_of(0.2 + 0.05 * i) for i in range(15)]
    down = up[::-1]
    hot_up = [[half_of(20.0 + 2.0 * i), half_of(2.0), half_of(0.01)] for i in range(15)]
    hot_down = hot_up[::-1]
    top = R.MAX_CODE
    blocks = [
        ("no_swap", _split_block(13, up, hot_down)),                          # both anchors the darkest of their subset (partition 13: rows 0-1 | rows 2-3)
        ("swap0", _split_block(13, down, hot_down)),                          # texel 0 the brightest of subset 0
        ("swap1_anchor15", _split_block(13, up, hot_up)),                     # texel 15, the last of subset 1, its brightest
        ("swap1_anchor2", _split_block(17, up, hot_down)),                    # partition 17: subset 1 = texels 1 2 3 7, anchor 2 its second brightest
        ("swap1_anchor8", _split_block(18, up, hot_down)),                    # partition 18: subset 1 = texels 8 12 13 14, anchor 8 its brightest
        ("swap_both", _split_block(13, down, hot_up)),
        ("equal_subset", _split_block(13, up, [[half_of(30.0), half_of(3.0), half_of(0.5)]])),
        ("zero", np.zeros((16, 3), np.int64)),                                # E1 = 0: stays one-region
        ("spread15_at10", spread_block(q10, 500, 505, 509, 515, 507)),        # case 0 still fits
        ("spread16_at10", spread_block(q10, 500, 505, 509, 516, 507)),        # left for case 14
        ("spread31_at7", spread_block(q7, 20, 30, 40, 51, 35)),               # case 1 still fits
        ("spread32_at7", spread_block(q7, 20, 30, 40, 52, 35)),               # left for case 30
        ("max_next_to_small", _split_block(13, up, [top])),                   # 65504: the all-ones code at 6 bits
        ("max_at10", _split_block(13, [top - 400, top - 300, top - 250], [top - 90, top])),
        ("max_at9", _split_block(13, [top - 800, top - 600, top - 500], [top - 180, top])),
        ("max_at7", _split_block(13, [top - 5000, top - 3500, top - 3000], [top - 900, top])),
    ]
    return blocks


CRAFTED_NAMES = [n for n, _ in crafted_blocks()]


def crafted_strip_f16():
    """the crafted blocks, then bc6h_ref's hostile row with its half-only patterns, as RGBA16F bits"""
    return np.concatenate([_level_of_blocks([b for _, b in crafted_blocks()]), R.hostile_blocks_f16()], axis=2)


def crafted_strip_f32():
    """the crafted blocks (the same values), then bc6h_ref's hostile fp32 row"""
    return np.concatenate([as_float32(_level_of_blocks([b for _, b in crafted_blocks()])), R.hostile_blocks()], axis=2)


CUBE_FACES = (1, 2, 3, 5, 12, 20, 68)


def cases():
    """(name, level): the cases of bc6h_ref.cases() the two-region tests use, the strips and the scene"""
    keep = {f"cube{n}_{f}" for n in CUBE_FACES for f in ("f32", "f16")} | {"flat20x12_f32", "flat20x12_f16"}
    out = [(n, lvl) for n, lvl in R.cases() if n in keep]
    strip = partition_strip()
    out += [("partitions_f16", strip), ("partitions_f32", as_float32(strip)), ("crafted_f16", crafted_strip_f16()),
            ("crafted_f32", crafted_strip_f32()), ("edge_scene", edge_scene(128))]
    return out
