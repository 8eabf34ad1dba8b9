#!/usr/bin/env python3
"""Records tests/golden/bc_crops.npz: BC1 / BC3 / BC5 blocks and what an independent decoder (Pillow) makes of them.

    python tools/gen_bc_golden.py <directory with the SunTemple .dds textures> [out.npz]

Entries (per image NAME: NAME_blocks uint8, NAME_format str, NAME_rgba uint8 [h][w][4]):
  basecolor64, specular64, emissive64   64 x 64 crops (16 x 16 blocks) of level 0 of three files, at the most varied block window
  tail8, tail4, tail2, tail1            the last four levels of the base colour file
  rand_bc3, rand_bc5                    32 x 32 images of random blocks
  header                                the first 128 bytes of the base colour file
Every image goes to Pillow through an in-memory DDS wrapper around exactly the recorded blocks; the crops are also checked against
Pillow's decode of the whole file.  Needs Pillow; the tests only read the .npz."""
import io
import os
import struct
import sys

import numpy as np
from PIL import Image

FILES = {"basecolor64": "M_FirePit_Inst_0_BaseColor.dds", "specular64": "M_FirePit_Inst_0_Specular.dds",
         "emissive64": "M_FirePit_Inst_nofire_0_Emissive.dds"}
FOURCC = {"bc1_rgba": b"DXT1", "bc3": b"DXT5", "bc5": b"ATI2"}
BLOCK = {"bc1_rgba": 8, "bc3": 16, "bc5": 16}


def dds_wrap(fmt, w, h, blocks):
    """A one-level legacy DDS file around `blocks`."""
    pf = struct.pack("<II4sIIIII", 32, 0x4, FOURCC[fmt], 0, 0, 0, 0, 0)
    head = struct.pack("<IIIIIII", 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000, h, w, len(blocks), 0, 1) + bytes(44) + pf + struct.pack("<IIIII", 0x1000, 0, 0, 0, 0)
    assert len(head) == 124
    return b"DDS " + head + bytes(blocks)


def pillow_decode(fmt, w, h, blocks):
    im = Image.open(io.BytesIO(dds_wrap(fmt, w, h, blocks)))
    im.load()
    a = np.asarray(im.convert("RGBA"))
    assert a.shape == (h, w, 4), a.shape
    return a


def read_dds(path):
    raw = open(path, "rb").read()
    assert raw[:4] == b"DDS " and raw[84:88] == b"DXT1", path
    h, w, mips = struct.unpack_from("<II", raw, 12) + struct.unpack_from("<I", raw, 28)
    levels, off = [], 128
    for m in range(max(1, mips)):
        lw, lh = max(1, w >> m), max(1, h >> m)
        n = ((lw + 3) // 4) * ((lh + 3) // 4) * 8
        levels.append((lw, lh, raw[off:off + n]))
        off += n
    assert off == len(raw), (path, off, len(raw))
    return raw, levels


def best_window(blocks, bw, bh, n=16):
    """block offset (bx, by) of the n x n window with the most distinct blocks (8-block grid)"""
    ids = np.unique(np.frombuffer(blocks, np.uint8).reshape(bh * bw, 8), axis=0, return_inverse=True)[1].reshape(bh, bw)
    best, arg = -1, (0, 0)
    for by in range(0, bh - n + 1, 8):
        for bx in range(0, bw - n + 1, 8):
            k = len(np.unique(ids[by:by + n, bx:bx + n]))
            if k > best:
                best, arg = k, (bx, by)
    return arg


def main():
    src = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "bc_crops.npz")
    rec = {}

    def put(name, fmt, w, h, blocks):
        rec[name + "_blocks"] = np.frombuffer(bytes(blocks), np.uint8)
        rec[name + "_format"] = np.array(fmt)
        rec[name + "_rgba"] = pillow_decode(fmt, w, h, blocks)

    for name, fn in FILES.items():
        path = os.path.join(src, fn)
        raw, levels = read_dds(path)
        w, h, blocks = levels[0]
        bw, bh = w // 4, h // 4
        bx, by = best_window(blocks, bw, bh)
        crop = np.frombuffer(blocks, np.uint8).reshape(bh, bw, 8)[by:by + 16, bx:bx + 16].tobytes()
        put(name, "bc1_rgba", 64, 64, crop)
        whole = np.asarray(Image.open(path).convert("RGBA"))
        assert np.array_equal(whole[4 * by:4 * by + 64, 4 * bx:4 * bx + 64], rec[name + "_rgba"]), name
        if name == "basecolor64":
            rec["header"] = np.frombuffer(raw[:128], np.uint8)
            for lw, lh, lb in levels[-4:]:
                assert lw == lh and lw in (8, 4, 2, 1)
                put(f"tail{lw}", "bc1_rgba", lw, lh, lb)
    rng = np.random.default_rng(0xBC)
    for fmt in ("bc3", "bc5"):
        put("rand_" + fmt, fmt, 32, 32, rng.integers(0, 256, 8 * 8 * BLOCK[fmt], dtype=np.uint8).tobytes())
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes;", ", ".join(sorted(k for k in rec if k.endswith("_rgba") or k == "header")))


if __name__ == "__main__":
    main()
