#!/usr/bin/env python3
"""K18 at its two-region quality (pbrk_bc6h_encode2: k_bc6h.hip, csrc/bc6h2_core.h) next to the one-region kernel in the same session, on the
sizes a bake has: one RGBA32F cube level of 4096^2, 1024^2 and 256^2 with the content of tools/bc6h_time.py.  Per size, back to back
on one stream with GPUX_SetLevelOverlap(0): host clock around `launches` launches that end in a device synchronise, per launch (median
of `--repeats` windows after a warm-up window), for both kernels, and their ratio.  The yardstick is K18 in this session.
Then a C4-size bake (2048^2 environment -> 4096^2 specular cube with 13 levels): every level encoded in one graph into device memory,
at both qualities (host clock around submit and wait).
Quality, on the CPU restatements (tests/bc6h_ref.py, tests/bc6h2_ref.py; the kernel's blocks are asserted to be the same bytes): per
level of a 128^2 prefiltered cube baked from synth_env(256), at both qualities, the total squared half-code error, the worst relative
error of a texel (components above 2^-10) and, at quality 1, the share of blocks per kind.
Needs the GPU; there is no fallback.
    python3 tools/bc6h2_time.py [--out profiles/bc6h_encode2.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vulkan-pbr-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import bc6h2_ref as R2  # noqa: E402
import bc6h_decode_ref as D  # noqa: E402
import bc6h_ref as R  # noqa: E402
import pbrhip  # noqa: E402
from pbrhip import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc6h_encode2.json"))
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

env2048 = synth.synth_env(2048, seed=0x5EED0004, workers=6)    # before the backend starts: built by forked workers
env256 = synth.synth_env(256, seed=0x5EED0256)
L = pbrhip.init(0)
L.GPUX_SetLevelOverlap(0)
F32 = 4                                                                       # PBRK_FMT_RGBA32F
out = {"what": "K18 two regions (pbrk_bc6h_encode2) against K18 (pbrk_bc6h_encode) in the same session, one RGBA32F cube level per launch, "
               "back to back on one stream", "cases": []}


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


rng = np.random.default_rng(18)
for n, launches in ((4096, 4), (1024, 40), (256, 400)):
    face = (0.05 + np.abs(rng.standard_normal((n, n, 4))) * np.linspace(0.2, 3.0, n)[None, :, None]).astype(np.float32)
    tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, n, n, pbrhip.TextureFlag_Cubemap, None)
    pbrhip.upload_mip(tex, 0, np.broadcast_to(face, (6, n, n, 4)))
    nbytes = R.level_bytes(n, n, 6)
    blocks = L.GPU_MakeBuffer(nbytes, pbrhip.BufferFlag_GPU, None)
    src_p, blocks_p = L.GPUX_TextureDevicePtr(tex, 0), L.GPUX_BufferDevicePtr(blocks)
    one = windows(lambda: L.pbrk_bc6h_encode(src_p, F32, n, n, 6, blocks_p, None), launches)
    two = windows(lambda: L.pbrk_bc6h_encode2(src_p, F32, n, n, 6, blocks_p, None), launches)
    if n == 256:                                                              # the timed launches computed the contract's bytes (one face: all six are equal)
        host = L.GPU_MakeBuffer(nbytes, pbrhip.BufferFlag_CPU, None)
        g = L.GPU_MakeGraph()
        L.GPU_OpCopyBufferToBuffer(g, blocks, host, 0, 0, nbytes)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        assert C.string_at(host.contents.data, nbytes) == R2.encode2(face[None]).tobytes() * 6
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(host)
    a, b = float(np.median(one)), float(np.median(two))
    out["cases"].append({"case": f"{n}^2 cube level", "blocks": nbytes // 16, "launches_per_window": launches,
                         "one_region_us": round(a, 2), "one_region_us_windows": [round(x, 2) for x in one],
                         "two_regions_us": round(b, 2), "two_regions_us_windows": [round(x, 2) for x in two],
                         "ratio": round(b / a, 2), "two_regions_ns_per_block": round(b * 1e3 / (nbytes // 16), 4)})
    L.GPU_DestroyBuffer(blocks); L.GPU_DestroyTexture(tex)


def bake(env, irr, lut, spec):
    env_tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, env.shape[1], env.shape[1], pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), irr, lut, spec)
    L.PBR_GenPrefilteredEnvMap(env_tex, maps.tex_specular_env_map, 1)
    L.GPU_WaitUntilIdle()
    return env_tex, maps


# ---- every level of a C4-size specular cube in one graph, both ways ----
env_tex, maps = bake(env2048, 128, 256, 4096)
spec = maps.tex_specular_env_map
levels = spec.contents.mip_level_count
sizes = [L.GPUX_BC6HMipBytes(spec, m) for m in range(levels)]
buf = L.GPU_MakeBuffer(sum(sizes), pbrhip.BufferFlag_GPU, None)
span = {0: [], 1: []}
for quality in (0, 1):
    g = L.GPU_MakeGraph()
    for _ in range(4):                                                        # run 0 warms up
        off = 0
        for m in range(levels):
            L.GPUX_OpEncodeBC6HEx(g, spec, m, buf, off, quality)
            off += sizes[m]
        L.GPU_WaitUntilIdle()
        t0 = time.perf_counter()
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        span[quality].append((time.perf_counter() - t0) * 1e3)
    L.GPU_DestroyGraph(g)
L.GPU_DestroyBuffer(buf)
out["c4_cube"] = {"what": "4096^2 specular cube of a 2048^2 environment, all 13 levels as BC6H in one graph into device memory",
                  "one_region_ms": [round(x, 3) for x in span[0][1:]], "two_regions_ms": [round(x, 3) for x in span[1][1:]],
                  "ratio": round(float(np.median(span[1][1:]) / np.median(span[0][1:])), 2)}
L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(env_tex)

# ---- quality on a real bake ----
env_tex, maps = bake(env256, 16, 16, 128)
quality = []
kinds = ("one_region", "case_0", "case_14", "case_1", "case_30")
for m in range(maps.tex_specular_env_map.contents.mip_level_count):
    level = pbrhip.read_mip(maps.tex_specular_env_map, m)
    h = R.block_texels(R.half_codes(level))
    n = int(level.shape[1])
    ref = level[..., :3].astype(np.float64)
    big = ref > 2.0 ** -10
    row = {"level": m, "size": n}
    blocks2, chosen = R2.encode2_blocks(h)
    for name, blocks, q in (("one_region", R.encode(level), 0), ("two_regions", blocks2, 1)):
        assert pbrhip.encode_bc6h(maps.tex_specular_env_map, m, q).tobytes() == blocks.tobytes()
        row[name + "_squared_half_code_error"] = int(((D.decode(blocks) - h) ** 2).sum())
        dec = D.decode_level_codes(blocks, n, n, 6).view(np.float16).astype(np.float64)
        row[name + "_worst_relative_error"] = round(float((np.abs(dec - ref)[big] / ref[big]).max()), 5) if big.any() else None
    row["error_ratio"] = round(row["two_regions_squared_half_code_error"] / max(1, row["one_region_squared_half_code_error"]), 4)
    counts = np.bincount(chosen["kind"], minlength=5)
    row["share_of_blocks"] = {k: round(float(c) / len(h), 4) for k, c in zip(kinds, counts)}
    quality.append(row)
out["quality"] = {"what": "128^2 prefiltered cube of synth_env(256), CPU restatements; the kernels' blocks are the same bytes", "levels": quality}
L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(env_tex)

print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
L.GPU_WaitUntilIdle(); L.GPU_Deinit()
