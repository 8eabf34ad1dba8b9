#!/usr/bin/env python3
"""K15 (BC decode) on the sizes the reference's assets have: 2048^2 and 512^2 BC1 (all 99 SunTemple textures are one of the two) and
2048^2 BC3.  Two numbers per case, named for what they are:
  back_to_back_us   host clock around `--launches` pbrk_bc_decode launches on one stream that end in a device synchronise, per launch
                    (median of `--repeats` windows after a warm-up window): the rate a loader that decodes many textures sees
  per_op_event_us   HIP-event time of the K15.bc_decode op that follows a GPUX_OpCopyBufferToTextureMip in a graph
                    (GPUX_EnableOpTiming; median over `--ops` ops)
and the bytes the algorithm moves (blocks read once, 4 B written per texel) as a fraction of 8 TB/s over the back-to-back time, next to
the project's K4a copy kernel (0.80 of 8 TB/s, README) as the yardstick.  Needs the GPU; there is no fallback.
    python3 tools/bc_decode_time.py [--out profiles/bc_decode.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vulkan-pbr-renderer_amd", "python"))
import numpy as np  # noqa: E402
import pbrhip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc_decode.json"))
ap.add_argument("--launches", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--ops", type=int, default=50)
args = ap.parse_args()

CASES = (("BC1 2048^2", pbrhip.Format_BC1_RGBA_UN, pbrhip.PBRK_BC1_RGBA, 2048), ("BC1 512^2", pbrhip.Format_BC1_RGBA_UN, pbrhip.PBRK_BC1_RGBA, 512),
         ("BC3 2048^2", pbrhip.Format_BC3_RGBA_UN, pbrhip.PBRK_BC3, 2048))
L = pbrhip.init(0)
rng = np.random.default_rng(15)
out = {"what": "K15 pbrk_bc_decode, one level per launch, random blocks", "yardstick_K4a_copy_fraction_of_8TBps": 0.80, "cases": []}
for name, fmt, kfmt, n in CASES:
    nbytes = (n // 4) ** 2 * pbrhip.BC_BLOCK_BYTES[fmt]
    blocks = rng.integers(0, 256, nbytes, dtype=np.uint8)
    tex = pbrhip.make_texture(fmt, n, n, 0, blocks)
    dst = pbrhip.make_texture(pbrhip.Format_RGBA8UN, n, n, 0, None)
    src_p, dst_p = L.GPUX_TextureDevicePtr(tex, 0), L.GPUX_TextureDevicePtr(dst, 0)
    windows = []
    for rep in range(args.repeats + 1):                                       # window 0 warms up
        L.GPU_WaitUntilIdle()
        t0 = time.perf_counter()
        for _ in range(args.launches):
            rc = L.pbrk_bc_decode(kfmt, src_p, n, n, dst_p, None)
            assert rc == 0, rc
        L.GPU_WaitUntilIdle()
        windows.append((time.perf_counter() - t0) / args.launches * 1e6)
    assert np.array_equal(pbrhip.read_mip(dst, 0), pbrhip.read_decoded_mip(tex, 0))       # the timed launches computed the texture's image
    staging = L.GPU_MakeBuffer(nbytes, pbrhip.BufferFlag_GPU, blocks.ctypes.data_as(C.c_void_p))
    g = L.GPU_MakeGraph()
    L.GPUX_EnableOpTiming(1)
    ev = []
    for rep in range(2):                                                      # submission 0 warms up
        for _ in range(args.ops):
            L.GPUX_OpCopyBufferToTextureMip(g, staging, 0, tex, 0)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        ev = [L.GPUX_GraphTimedOpMs(g, i) * 1e3 for i in range(L.GPUX_GraphTimedOpCount(g)) if L.GPUX_GraphTimedOpName(g, i) == b"K15.bc_decode"]
    L.GPUX_EnableOpTiming(0)
    assert len(ev) == args.ops, len(ev)
    moved = nbytes + 4 * n * n
    b2b = float(np.median(windows[1:]))
    out["cases"].append({"case": name, "bytes_read": nbytes, "bytes_written": 4 * n * n, "bytes_moved": moved,
                         "back_to_back_us": round(b2b, 3), "back_to_back_us_windows": [round(x, 3) for x in windows[1:]], "launches_per_window": args.launches,
                         "per_op_event_us": round(float(np.median(ev)), 3), "per_op_event_us_min": round(float(min(ev)), 3),
                         "hbm_floor_us": round(moved / 8e12 * 1e6, 3), "fraction_of_8TBps": round(moved / (b2b * 1e-6) / 8e12, 4)})
    L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(staging); L.GPU_DestroyTexture(tex); L.GPU_DestroyTexture(dst)
print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
L.GPU_WaitUntilIdle(); L.GPU_Deinit()
