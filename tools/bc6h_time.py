#!/usr/bin/env python3
"""K18 (BC6H encode) on the sizes a bake has: one RGBA32F cube level of 4096^2, 1024^2 and 256^2.  Per size, back to back on one stream
with GPUX_SetLevelOverlap(0):
  encode_us       host clock around `launches` pbrk_bc6h_encode launches that end in a device synchronise, per launch (median of
                  `--repeats` windows after a warm-up window)
  k4a_copy_us     the same for K4a's copy of the same level (pbrk_prefilter_copy, n -> n): the project's bandwidth floor, same session
and the bytes the encode must move (16 B read, 1 B written per texel) as a fraction of 8 TB/s over encode_us.
Then a C4-size bake (2048^2 environment -> 4096^2 specular cube with 13 levels + 128^2 irradiance): the bake's own time next to the
time to encode every level as BC6H in one graph into device memory (host clock around submit and wait) and to produce the whole .dds in memory (PBR_EncodeTextureDDS, host
clock: encode into mapped memory + the face-major reorder), so a reader sees what saving costs.
Quality, on the CPU restatement (tests/bc6h_ref.py): per level of a 128^2 prefiltered cube baked from a synth environment, the total
squared half-code error of encode and of encode_bbox and the worst relative error of a texel (components above 2^-10).
Needs the GPU; there is no fallback.
    python3 tools/bc6h_time.py [--out profiles/bc6h_encode.json]"""
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
import bc6h_ref as R  # noqa: E402
import pbrhip  # noqa: E402
from pbrhip import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc6h_encode.json"))
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

env2048 = synth.synth_env(2048, seed=0x5EED0004, workers=6)    # before the backend starts: built by forked workers
env256 = synth.synth_env(256, seed=0x5EED0256)
L = pbrhip.init(0)
L.GPUX_SetLevelOverlap(0)
F32 = 4                                                                       # PBRK_FMT_RGBA32F
out = {"what": "K18 pbrk_bc6h_encode, one RGBA32F cube level per launch, back to back on one stream", "cases": []}


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
for n, launches in ((4096, 10), (1024, 100), (256, 1000)):
    face = (0.05 + np.abs(rng.standard_normal((n, n, 4))) * np.linspace(0.2, 3.0, n)[None, :, None]).astype(np.float32)
    tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, n, n, pbrhip.TextureFlag_Cubemap, None)
    pbrhip.upload_mip(tex, 0, np.broadcast_to(face, (6, n, n, 4)))
    copy = pbrhip.make_texture(pbrhip.Format_RGBA32F, n, n, pbrhip.TextureFlag_Cubemap, None)
    nbytes = R.level_bytes(n, n, 6)
    blocks = L.GPU_MakeBuffer(nbytes, pbrhip.BufferFlag_GPU, None)
    bord = L.GPU_MakeBuffer(L.pbrk_bordered_pyramid_texels(n, 1) * 16, pbrhip.BufferFlag_GPU, None)
    src_p, copy_p, blocks_p, bord_p = L.GPUX_TextureDevicePtr(tex, 0), L.GPUX_TextureDevicePtr(copy, 0), L.GPUX_BufferDevicePtr(blocks), L.GPUX_BufferDevicePtr(bord)
    assert L.pbrk_border_build(src_p, bord_p, n, 1, None) == 0
    enc = windows(lambda: L.pbrk_bc6h_encode(src_p, F32, n, n, 6, blocks_p, None), launches)
    cpy = windows(lambda: L.pbrk_prefilter_copy(bord_p, n, copy_p, n, 0, 6, 0, n, None), launches)
    if n == 256:                                                              # the timed launches computed the contract's bytes
        host = L.GPU_MakeBuffer(nbytes, pbrhip.BufferFlag_CPU, None)
        g = L.GPU_MakeGraph()
        L.GPU_OpCopyBufferToBuffer(g, blocks, host, 0, 0, nbytes)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        assert C.string_at(host.contents.data, nbytes) == R.encode(np.broadcast_to(face, (6, n, n, 4))).tobytes()
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(host)
    moved = 6 * n * n * 17
    e, c = float(np.median(enc)), float(np.median(cpy))
    out["cases"].append({"case": f"{n}^2 cube level", "blocks": nbytes // 16, "bytes_moved": moved, "launches_per_window": launches,
                         "encode_us": round(e, 2), "encode_us_windows": [round(x, 2) for x in enc],
                         "k4a_copy_us": round(c, 2), "k4a_copy_us_windows": [round(x, 2) for x in cpy], "k4a_copy_bytes_moved": 6 * n * n * 32,
                         "hbm_floor_us": round(moved / 8e12 * 1e6, 2), "fraction_of_8TBps": round(moved / (e * 1e-6) / 8e12, 4),
                         "k4a_copy_fraction_of_8TBps": round(6 * n * n * 32 / (c * 1e-6) / 8e12, 4),
                         "ns_per_block": round(e * 1e3 / (nbytes // 16), 4)})
    for b in (blocks, bord):
        L.GPU_DestroyBuffer(b)
    L.GPU_DestroyTexture(tex); L.GPU_DestroyTexture(copy)


def bake(env, irr, lut, spec):
    env_tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, env.shape[1], env.shape[1], pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), irr, lut, spec)
    times = []
    for _ in range(3):                                                        # run 0 warms up
        L.GPU_WaitUntilIdle()
        t0 = time.perf_counter()
        L.PBR_GenPrefilteredEnvMap(env_tex, maps.tex_specular_env_map, 1)
        L.PBR_GenIrradianceMap(env_tex, maps.irradiance_map)
        L.GPU_WaitUntilIdle()
        times.append((time.perf_counter() - t0) * 1e3)
    return env_tex, maps, times[1:]


# ---- the C4-size bake and what saving it costs ----
env_tex, maps, bake_ms = bake(env2048, 128, 256, 4096)
spec = maps.tex_specular_env_map
levels = spec.contents.mip_level_count
sizes = [L.GPUX_BC6HMipBytes(spec, m) for m in range(levels)]
buf = L.GPU_MakeBuffer(sum(sizes), pbrhip.BufferFlag_GPU, None)
g = L.GPU_MakeGraph()
span = []
for _ in range(4):
    off = 0
    for m in range(levels):
        L.GPUX_OpEncodeBC6H(g, spec, m, buf, off)
        off += sizes[m]
    L.GPU_WaitUntilIdle()
    t0 = time.perf_counter()
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    span.append((time.perf_counter() - t0) * 1e3)
L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(buf)
whole = []
for _ in range(3):
    t0 = time.perf_counter()
    size = C.c_size_t(0)
    p = L.PBR_EncodeTextureDDS(spec, 0, 0, pbrhip.PBR_DDS_OUT_BC6H_UF16, C.byref(size))
    whole.append((time.perf_counter() - t0) * 1e3)
    assert p and size.value
    pbrhip._libc_free(p)
out["c4_bake"] = {"what": "2048^2 environment -> 4096^2 specular cube (13 levels) + 128^2 irradiance; then the specular cube as BC6H",
                  "bake_ms": [round(x, 2) for x in bake_ms], "bc6h_all_levels_one_graph_ms": [round(x, 3) for x in span[1:]],
                  "encode_texture_dds_host_ms": [round(x, 1) for x in whole[1:]], "dds_bytes": int(size.value),
                  "rgba32f_bytes": int(sum(L.GPUX_TextureMipBytes(spec, m) for m in range(levels)))}
L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(env_tex)

env_tex, maps, _ = bake(env256, 16, 16, 128)
quality = []
for m in range(maps.tex_specular_env_map.contents.mip_level_count):
    level = pbrhip.read_mip(maps.tex_specular_env_map, m)
    h = R.block_texels(R.half_codes(level))
    row = {"level": m, "size": int(level.shape[1])}
    for name, blocks in (("encode", R.encode(level)), ("encode_bbox", R.encode_bbox(level))):
        row[name + "_squared_half_code_error"] = int(((R.decode(blocks) - h) ** 2).sum())
    assert pbrhip.encode_bc6h(maps.tex_specular_env_map, m).tobytes() == R.encode(level).tobytes()
    dec = R.decode_level(R.encode(level), level.shape[2], level.shape[1], 6)
    ref = level[..., :3].astype(np.float64)
    big = ref > 2.0 ** -10
    row["worst_relative_error"] = round(float((np.abs(dec - ref)[big] / ref[big]).max()), 5) if big.any() else None
    quality.append(row)
out["quality"] = {"what": "128^2 prefiltered cube of synth_env(256), CPU restatement; the kernel's blocks are the same bytes", "levels": quality}
L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(env_tex)

print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
L.GPU_WaitUntilIdle(); L.GPU_Deinit()
