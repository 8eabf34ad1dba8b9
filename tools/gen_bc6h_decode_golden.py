#!/usr/bin/env python3
"""Records tests/golden/bc6h_modes_pillow.npz: random BC6H_UF16 blocks of every mode value and what an independent decoder (Pillow)
makes of them.

    python tools/gen_bc6h_decode_golden.py [out.npz]

Entries, for each of the 18 values M the mode bits can take (the 14 modes and the reserved 19, 23, 27, 31):
  modeM_blocks  uint8 [64][16]   random bytes with the mode bits forced (tests/bc6h_decode_ref.py random_blocks, seed 0xBC6D00 + M)
  modeM_rgb     uint8 [32][32][3] Pillow's decode of those blocks as one 32 x 32 image
Every image goes to Pillow through an in-memory DX10 DDS (DXGI 95), as tools/gen_bc6h_golden.py does.  Before anything is written the
restatement is held against Pillow per mode: max difference <= 1 code, share of equal values >= 0.995, share of values strictly inside
(0, 255) >= 0.15 for the valid modes, reserved modes all zero.  Needs Pillow; the tests only read the .npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bc6h_decode_ref as D  # noqa: E402
from gen_bc6h_golden import pillow_decode  # noqa: E402

SEED = 0xBC6D00


def quantized(blocks):
    """the restatement's 32 x 32 image the way tests/test_bc6h_core_host.py quantises: floor(clamp(v, 0, 1) * 255)"""
    v = D.decode_level_codes(blocks, 32, 32, 1)[0].view(np.float16).astype(np.float32)
    return np.floor(np.clip(v, 0.0, 1.0) * 255.0).astype(np.int64)


def check(mode, got, want):
    """the conditions of the fixture; returns (max difference, share equal, share inside)"""
    diff = np.abs(got - want)
    equal = float((diff == 0).mean())
    inside = float(((want > 0) & (want < 255)).mean())
    assert diff.max() <= 1, (mode, int(diff.max()))
    assert equal >= 0.995, (mode, equal)
    if mode in D.RESERVED:
        assert not got.any() and not want.any(), mode
    else:
        assert inside >= 0.15, (mode, inside)
    return int(diff.max()), equal, inside


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "bc6h_modes_pillow.npz")
    rec = {}
    for mode in D.MODE_VALUES:
        blocks = D.random_blocks(64, SEED + mode, mode)
        rgb = pillow_decode(32, 32, blocks.tobytes())
        print("mode %2d: max %d equal %.4f inside %.3f" % ((mode,) + check(mode, quantized(blocks), rgb.astype(np.int64))))
        rec[f"mode{mode}_blocks"] = blocks
        rec[f"mode{mode}_rgb"] = rgb
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 100 * 1024


if __name__ == "__main__":
    main()
