#!/usr/bin/env python3
"""Records tests/golden/bc6h_pillow.npz: BC6H blocks from the encode contract (tests/bc6h_ref.py) and what an independent decoder
(Pillow) makes of them.

    python tools/gen_bc6h_golden.py [out.npz]

Entries (per image NAME: NAME_blocks uint8 [n][16], NAME_size [w, h], NAME_rgb uint8 [h][w][3]):
  smooth32   32 x 32 of smooth HDR content with texels far above 1 (Pillow saturates them to 255: the endpoints' top bits)
  hostile    the crafted row of hostile blocks
  bright16   16 x 16 with every texel between 0.02 and 4
Every image goes to Pillow through an in-memory DX10 DDS (DXGI 95, BC6H_UF16) around exactly the recorded blocks.  Needs Pillow; the
tests only read the .npz."""
import io
import os
import struct
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bc6h_ref as R  # noqa: E402


def dds_wrap(w, h, blocks):
    """A one-level DX10 DDS file around `blocks`."""
    pf = struct.pack("<II4sIIIII", 32, 0x4, b"DX10", 0, 0, 0, 0, 0)
    head = struct.pack("<IIIIIII", 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000, h, w, len(blocks), 0, 1) + bytes(44) + pf + struct.pack("<IIIII", 0x1000, 0, 0, 0, 0)
    assert len(head) == 124
    return b"DDS " + head + struct.pack("<IIIII", 95, 3, 0, 1, 0) + bytes(blocks)


def pillow_decode(w, h, blocks):
    im = Image.open(io.BytesIO(dds_wrap(w, h, blocks)))
    im.load()
    a = np.asarray(im.convert("RGB"))
    assert a.shape == (h, w, 3), a.shape
    return a


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "bc6h_pillow.npz")
    rng = np.random.default_rng(0xBC6)
    bright = np.ones((1, 16, 16, 4), np.float32)
    bright[..., :3] = np.exp(rng.uniform(np.log(0.02), np.log(4.0), (1, 16, 16, 3)))
    smooth = R.hdr_level(32, 32, 1, 32)
    smooth[..., :3] *= 0.25
    rec, texels = {}, 0
    for name, lvl in (("smooth32", smooth), ("hostile", R.hostile_blocks()), ("bright16", bright)):
        _, h, w, _ = lvl.shape
        blocks = R.encode(lvl)
        rec[name + "_blocks"] = blocks
        rec[name + "_size"] = np.array([w, h])
        rec[name + "_rgb"] = pillow_decode(w, h, blocks.tobytes())
        texels += w * h
    assert texels <= 64 * 64
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes;", texels, "texels")


if __name__ == "__main__":
    main()
