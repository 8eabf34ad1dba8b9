#!/usr/bin/env python3
"""K21 (GGX importance-sampled prefilter) on the C4 shape: levels 1 .. 12 of a 4096^2 specular cube from a 2048^2 environment with its
chain, at N = 64, 256 and 1024 samples per texel, beside the unchanged K4b job in the same session, level overlap off.
  k4b_job_ms      host clock around PBR_GenPrefilteredEnvMap (blocking: level 0's copy and levels 1 .. 12 by K4b), median of `--repeats`
                  runs after two warm-up runs (the first run of a process bins the tiles)
  ggx_job_ms      the same around PBR_GenPrefilteredEnvMapGGX (the same copy, levels 1 .. 12 by K21), after one warm-up run
  levels          per level of the K21 job its event time inside one graph of the twelve ops (median of `--repeats` submissions), the kept
                  samples, how many of them blend two source levels, and the VALU issue floor of that level: texels x (85 VALU
                  instructions per one-level sample, 121 per two-level sample: counted in the kernel's loop, profiles/prefilter_ggx.md)
                  x 4 cycles per wave instruction over 1024 SIMDs at 2.4 GHz
Needs the GPU; there is no fallback.
    python3 tools/prefilter_ggx_time.py [--out profiles/prefilter_ggx.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vulkan-pbr-renderer_amd", "python"))
import numpy as np  # noqa: E402
import pbrhip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefilter_ggx.json"))
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--env", type=int, default=2048)
ap.add_argument("--spec", type=int, default=4096)
args = ap.parse_args()

VALU_ONE, VALU_TWO, SIMDS, HZ = 85, 121, 1024, 2.4e9

L = pbrhip.init(0)
L.GPUX_SetLevelOverlap(0)
rng = np.random.default_rng(21)
env_data = np.exp(1.5 * rng.standard_normal((6, args.env, args.env, 4), dtype=np.float32))
env = pbrhip.make_texture(pbrhip.Format_RGBA32F, args.env, args.env, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env_data)
del env_data
spec = pbrhip.make_texture(pbrhip.Format_RGBA32F, args.spec, args.spec,
                           pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps | pbrhip.TextureFlag_StorageImage)
levels = spec.contents.mip_level_count


def clocked(job, warm):
    t = []
    for k in range(warm + args.repeats):
        L.GPU_WaitUntilIdle()
        t0 = time.perf_counter()
        job()
        L.GPU_WaitUntilIdle()
        if k >= warm:
            t.append((time.perf_counter() - t0) * 1e3)
    return t


out = {"what": f"K21 on the C4 shape: levels 1 .. {levels - 1} of a {args.spec}^2 cube from a {args.env}^2 environment, level overlap off",
       "valu_per_sample": [VALU_ONE, VALU_TWO], "jobs": []}
k4b = clocked(lambda: L.PBR_GenPrefilteredEnvMap(env, spec, 1), 2)
out["k4b_job_ms"] = round(float(np.median(k4b)), 3)
out["k4b_job_ms_runs"] = [round(x, 3) for x in k4b]

for count in (64, 256, 1024):
    job = clocked(lambda: L.PBR_GenPrefilteredEnvMapGGX(env, spec, 1, count), 1)
    L.GPUX_EnableOpTiming(1)
    g = L.GPU_MakeGraph()
    per_level, spans = {}, []
    for _ in range(args.repeats):
        for i in range(1, levels):
            L.GPUX_OpPrefilterGGX(g, env, spec, i, min(1.0, i / 4), count, 1.0, 0, 6, 0, max(1, args.spec >> i))
        L.GPU_GraphSubmit(g)
        L.GPU_GraphWait(g)
        spans.append(L.GPUX_GraphSpanMs(g))
        for k in range(L.GPUX_GraphTimedOpCount(g)):
            per_level.setdefault(L.GPUX_GraphTimedOpName(g, k).decode(), []).append(L.GPUX_GraphTimedOpMs(g, k))
    L.GPU_DestroyGraph(g)
    L.GPUX_EnableOpTiming(0)
    rows = []
    for i in range(1, levels):
        size = max(1, args.spec >> i)
        table, _ = pbrhip.prefilter_ggx_samples(min(1.0, i / 4), count, args.env, env.contents.mip_level_count, 1.0)
        lod = table[:, 3]
        two = int((np.minimum(np.floor(lod) + 1, env.contents.mip_level_count - 1) != np.floor(lod)).sum())
        ms = float(np.median(per_level[f"K21.prefilter_ggx.mip{i}"]))
        floor_ms = 6.0 * size * size / 64 * (VALU_ONE * (len(table) - two) + VALU_TWO * two) * 4 / (SIMDS * HZ) * 1e3
        rows.append({"mip": i, "size": size, "roughness": min(1.0, i / 4), "kept": len(table), "two_level_samples": two,
                     "lod_min": round(float(lod.min()), 2), "lod_max": round(float(lod.max()), 2), "ms": round(ms, 4),
                     "ns_per_texel_sample": round(ms * 1e6 / (6.0 * size * size * len(table)), 5),
                     "valu_issue_floor_ms": round(floor_ms, 4), "fraction_of_valu_floor": round(floor_ms / ms, 3)})
    out["jobs"].append({"samples": count, "ggx_job_ms": round(float(np.median(job)), 3), "ggx_job_ms_runs": [round(x, 3) for x in job],
                        "graph_span_ms": round(float(np.median(spans)), 3), "k4b_over_ggx": round(out["k4b_job_ms"] / float(np.median(job)), 2),
                        "levels": rows})

print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
L.GPU_DestroyTexture(spec); L.GPU_DestroyTexture(env)
L.GPU_WaitUntilIdle(); L.GPU_Deinit()
