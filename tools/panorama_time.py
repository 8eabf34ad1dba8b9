#!/usr/bin/env python3
"""K20 (cube level -> lat-long panorama) on the sizes a bake has: the 4 n x 2 n panorama of a 1024^2 and of a 256^2 cube level into RGBA32F
and into RGBA16F.  Per size, back to back on one stream:
  panorama_us     host clock around `launches` pbrk_cube_to_panorama launches that end in a device synchronise, per launch (median of
                  `--repeats` windows after a warm-up window); the apron is built before and is not in it
  apron_us        the same for pbrk_border_build of that level, which the op runs first when the cube has no valid apron
  k4a_copy_us     the same for K4a's copy of the same level (pbrk_prefilter_copy, n -> n): the project's usual streaming yardstick, same session
and the bytes K20 must move -- 16 or 8 B per pixel written, the bordered level read once at 96 (n + 2)^2 B -- as a fraction of 8 TB/s over
panorama_us.  The 256^2 case is held against the numpy restatement (tests/panorama_ref.py) in both targets.
Needs the GPU; there is no fallback.
    python3 tools/panorama_time.py [--out profiles/panorama.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vulkan-pbr-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import panorama_ref as P  # noqa: E402
import pbrhip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panorama.json"))
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

L = pbrhip.init(0)
L.GPUX_SetLevelOverlap(0)
F32, F16 = 4, 3                                                               # PBRK_FMT_*
out = {"what": "K20 pbrk_cube_to_panorama, one 4n x 2n panorama per launch, back to back on one stream", "cases": []}


def windows(launch, launches):
    w = []
    for _ in range(args.repeats + 1):                                         # window 0 warms up
        L.GPU_WaitUntilIdle()
        t0 = time.perf_counter()
        for _ in range(launches):
            assert launch() == 0
        L.GPU_WaitUntilIdle()
        w.append((time.perf_counter() - t0) / launches * 1e6)
    return w[1:]


rng = np.random.default_rng(20)
for n, launches in ((1024, 200), (256, 1000)):
    w, h = 4 * n, 2 * n
    level = np.exp(rng.normal(0.0, 1.5, (6, n, n, 4))).astype(np.float32)
    tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, n, n, pbrhip.TextureFlag_Cubemap, None)
    pbrhip.upload_mip(tex, 0, level)
    copy_out = pbrhip.make_texture(pbrhip.Format_RGBA32F, n, n, pbrhip.TextureFlag_Cubemap, None)
    out32 = pbrhip.make_texture(pbrhip.Format_RGBA32F, w, h, 0, None)
    out16 = pbrhip.make_texture(pbrhip.Format_RGBA16F, w, h, 0, None)
    # the table as pano_fill_table lays it out (numpy's cos / sin: the timing does not depend on their last bit, and the check below
    # forms its directions from this very table)
    phi = ((2 * np.arange(w, dtype=np.float64) + 1) / w - 1) * np.pi
    theta = (2 * np.arange(h, dtype=np.float64) + 1) / (2 * h) * np.pi
    cols, rows = np.stack([np.cos(phi), np.sin(phi)], -1), np.stack([np.sin(theta), np.cos(theta)], -1)
    table_host = np.ascontiguousarray(np.concatenate([cols.ravel(), rows.ravel()]))
    table = L.GPU_MakeBuffer(table_host.nbytes, pbrhip.BufferFlag_GPU, table_host.ctypes.data_as(pbrhip.VP))
    bord = L.GPU_MakeBuffer(L.pbrk_bordered_pyramid_texels(n, 1) * 16, pbrhip.BufferFlag_GPU, None)
    src_p, copy_p, out32_p, out16_p = (L.GPUX_TextureDevicePtr(t, 0) for t in (tex, copy_out, out32, out16))
    table_p, bord_p = L.GPUX_BufferDevicePtr(table), L.GPUX_BufferDevicePtr(bord)
    assert L.pbrk_border_build(src_p, bord_p, n, 1, None) == 0
    L.GPU_WaitUntilIdle()
    apron = windows(lambda: L.pbrk_border_build(src_p, bord_p, n, 1, None), launches)
    cpy = windows(lambda: L.pbrk_prefilter_copy(bord_p, n, copy_p, n, 0, 6, 0, n, None), launches)
    a, c = float(np.median(apron)), float(np.median(cpy))
    read = 96 * (n + 2) * (n + 2)
    for fmt, fmt_name, dst, dst_p, texel in ((F32, "RGBA32F", out32, out32_p, 16), (F16, "RGBA16F", out16, out16_p, 8)):
        pan = windows(lambda: L.pbrk_cube_to_panorama(bord_p, n, table_p, dst_p, fmt, w, h, None), launches)
        if n == 256:                                                          # the timed launches computed the contract's values
            dirs = np.stack([(rows[:, None, 0] * cols[None, :, 0]).astype(np.float32), (rows[:, None, 0] * cols[None, :, 1]).astype(np.float32),
                             np.broadcast_to(rows[:, None, 1].astype(np.float32), (h, w))], -1)
            want = P.sample(level, dirs)
            got = pbrhip.read_mip(dst, 0)
            assert got.tobytes() == (want if fmt == F32 else want.astype(np.float16)).tobytes()
        moved = read + w * h * texel
        p = float(np.median(pan))
        out["cases"].append({"case": f"{w} x {h} panorama of a {n}^2 cube level", "target": fmt_name, "bytes_written": w * h * texel, "bytes_read_once": read,
                             "bytes_moved": moved, "launches_per_window": launches, "panorama_us": round(p, 2), "panorama_us_windows": [round(x, 2) for x in pan],
                             "apron_us": round(a, 2), "apron_us_windows": [round(x, 2) for x in apron],
                             "k4a_copy_us": round(c, 2), "k4a_copy_us_windows": [round(x, 2) for x in cpy], "k4a_copy_bytes_moved": 6 * n * n * 32,
                             "panorama_over_copy": round(p / c, 3), "hbm_floor_us": round(moved / 8e12 * 1e6, 2),
                             "fraction_of_8TBps": round(moved / (p * 1e-6) / 8e12, 4),
                             "k4a_copy_fraction_of_8TBps": round(6 * n * n * 32 / (c * 1e-6) / 8e12, 4)})
    for b in (table, bord):
        L.GPU_DestroyBuffer(b)
    for t in (tex, copy_out, out32, out16):
        L.GPU_DestroyTexture(t)

print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
L.GPU_WaitUntilIdle(); L.GPU_Deinit()
