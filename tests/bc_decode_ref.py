"""Numpy restatement of the K15 decode contract (csrc/bc_core.h), independent of the C++ header: BC1 / BC3 / BC5
blocks -> RGBA8.  Integer arithmetic; endpoints widened by bit replication; interpolants with truncating division.

Also the block sets the CPU and GPU tests share: the extents, random blocks (which reach every mode) and crafted blocks."""
import numpy as np

FORMATS = ("bc1_rgb", "bc1_rgba", "bc3", "bc5")
BLOCK_BYTES = {"bc1_rgb": 8, "bc1_rgba": 8, "bc3": 16, "bc5": 16}
KERNEL_FORMAT = {"bc1_rgb": 0, "bc1_rgba": 1, "bc3": 2, "bc5": 3}           # PBRK_BC1_RGB .. PBRK_BC5 / BC_FMT_*
EXTENTS = ((1, 1), (2, 2), (3, 5), (4, 4), (5, 4), (7, 9), (64, 64))         # (width, height)


def blocks_shape(w, h):
    return (h + 3) // 4, (w + 3) // 4


def level_bytes(fmt, w, h):
    bh, bw = blocks_shape(w, h)
    return bh * bw * BLOCK_BYTES[fmt]


def _color_blocks(b, four_only, punch):
    """b: uint8 [n][8] -> uint8 [n][16 texels][4]"""
    b = b.astype(np.int64)
    c0 = b[:, 0] | (b[:, 1] << 8)
    c1 = b[:, 2] | (b[:, 3] << 8)

    def rgb(c):
        r, g, bl = (c >> 11) & 31, (c >> 5) & 63, c & 31
        return np.stack([(r << 3) | (r >> 2), (g << 2) | (g >> 4), (bl << 3) | (bl >> 2)], -1)

    p0, p1 = rgb(c0), rgb(c1)
    four = (c0 > c1) | four_only
    pal = np.zeros((len(b), 4, 4), np.int64)
    pal[:, 0, :3], pal[:, 1, :3] = p0, p1
    pal[:, :, 3] = 255
    pal[:, 2, :3] = np.where(four[:, None], (2 * p0 + p1) // 3, (p0 + p1) // 2)
    pal[:, 3, :3] = np.where(four[:, None], (p0 + 2 * p1) // 3, 0)
    if punch:
        pal[:, 3, 3] = np.where(four, 255, 0)
    bits = b[:, 4] | (b[:, 5] << 8) | (b[:, 6] << 16) | (b[:, 7] << 24)
    idx = (bits[:, None] >> (2 * np.arange(16))[None, :]) & 3
    return np.take_along_axis(pal, idx[:, :, None].repeat(4, 2), 1).astype(np.uint8)


def _alpha_blocks(b):
    """b: uint8 [n][8] -> uint8 [n][16 texels]"""
    b = b.astype(np.int64)
    a0, a1 = b[:, 0], b[:, 1]
    big = a0 > a1
    pal = np.zeros((len(b), 8), np.int64)
    pal[:, 0], pal[:, 1] = a0, a1
    for i in range(1, 7):
        seven = ((7 - i) * a0 + i * a1) // 7
        five = ((5 - i) * a0 + i * a1) // 5 if i <= 4 else np.full_like(a0, 0 if i == 5 else 255)
        pal[:, i + 1] = np.where(big, seven, five)
    bits = np.zeros(len(b), np.int64)
    for k in range(6):
        bits |= b[:, 2 + k] << (8 * k)
    idx = (bits[:, None] >> (3 * np.arange(16))[None, :]) & 7
    return np.take_along_axis(pal, idx, 1).astype(np.uint8)


def decode(fmt, blocks, w, h):
    """blocks: bytes or uint8 array of ceil(w/4) x ceil(h/4) blocks, row major -> uint8 [h][w][4]; texels outside the level are dropped."""
    bh, bw = blocks_shape(w, h)
    nb = BLOCK_BYTES[fmt]
    b = np.frombuffer(bytes(blocks), np.uint8) if not isinstance(blocks, np.ndarray) else blocks.astype(np.uint8).ravel()
    assert b.size == bh * bw * nb, (b.size, bh, bw, nb)
    b = b.reshape(bh * bw, nb)
    if fmt in ("bc1_rgb", "bc1_rgba"):
        tex = _color_blocks(b, False, fmt == "bc1_rgba")
    elif fmt == "bc3":
        tex = _color_blocks(b[:, 8:], True, False)
        tex[:, :, 3] = _alpha_blocks(b[:, :8])
    elif fmt == "bc5":
        tex = np.zeros((bh * bw, 16, 4), np.uint8)
        tex[:, :, 0] = _alpha_blocks(b[:, :8])
        tex[:, :, 1] = _alpha_blocks(b[:, 8:])
        tex[:, :, 3] = 255
    else:
        raise ValueError(fmt)
    img = tex.reshape(bh, bw, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(bh * 4, bw * 4, 4)
    return np.ascontiguousarray(img[:h, :w])


def random_blocks(fmt, w, h, seed):
    """Uniformly random bytes: every mode (c0 > / == / < c1 is rare only for ==, see crafted_blocks), every index."""
    return np.random.default_rng(seed).integers(0, 256, level_bytes(fmt, w, h), dtype=np.uint8)


def _color_block(c0, c1, rows=(0xE4, 0x1B, 0xFF, 0x00)):       # 0xE4: indices 0 1 2 3; 0x1B: 3 2 1 0; 0xFF: all 3
    return [c0 & 255, c0 >> 8, c1 & 255, c1 >> 8, *rows]


def _alpha_block(a0, a1, second_half=False):
    idx = list(range(8)) * 2 if not second_half else [6, 7] * 8
    bits = sum(v << (3 * k) for k, v in enumerate(idx))
    return [a0, a1] + [(bits >> (8 * k)) & 255 for k in range(6)]


def crafted_blocks(fmt):
    """-> (blocks uint8, width, height): one row of blocks.  Colour: c0 > c1, c0 == c1, c0 < c1 (each with index 3 in use), endpoints
    0 and 0xFFFF.  Alpha / channel: a0 > a1, a0 <= a1 with indices 6 and 7, endpoints 0 and 255."""
    colors = [_color_block(0xF81F, 0x07E0), _color_block(0x1234, 0x1234), _color_block(0x07E0, 0xF81F), _color_block(0x0000, 0xFFFF),
              _color_block(0xFFFF, 0x0000), _color_block(0x0000, 0x0000), _color_block(0xFFFF, 0xFFFF), _color_block(0x8410, 0x8411)]
    alphas = [_alpha_block(200, 13), _alpha_block(13, 200), _alpha_block(13, 200, True), _alpha_block(77, 77), _alpha_block(0, 255),
              _alpha_block(255, 0), _alpha_block(0, 0, True), _alpha_block(255, 255)]
    if fmt in ("bc1_rgb", "bc1_rgba"):
        blocks = colors
    elif fmt == "bc3":
        blocks = [a + c for a, c in zip(alphas, colors)]
    else:
        blocks = [a + b for a, b in zip(alphas, alphas[1:] + alphas[:1])]
    return np.array(blocks, np.uint8).ravel(), 4 * len(blocks), 4


def cases():
    """[(name, fmt, width, height, blocks)]: every extent with random blocks and the crafted row, per format."""
    out = []
    for f, fmt in enumerate(FORMATS):
        for k, (w, h) in enumerate(EXTENTS):
            out.append((f"{fmt}-{w}x{h}", fmt, w, h, random_blocks(fmt, w, h, 1000 + 16 * f + k)))
        b, w, h = crafted_blocks(fmt)
        out.append((f"{fmt}-crafted", fmt, w, h, b))
    return out
