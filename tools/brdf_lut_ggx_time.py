#!/usr/bin/env python3
"""K22 (GGX split-sum BRDF LUT) on the C1 shape: a 256 x 256 RG16F map at N = 64, 1024 and 4096 samples per texel, both visibility
terms, and K1's 256 x 256 map at the reference's 4096 samples, all seven ops back to back in one graph on one stream.
  ops             per op its event time inside the graph (median of `--repeats` submissions after one warm-up submission), the time per
                  texel and sample, and for K22 the VALU issue floor: texels / 64 x N x (29 VALU instructions per sample for
                  Smith-Schlick, 48 for the correlated term: counted in the kernel's loop, profiles/brdf_lut_ggx.md) x 4 cycles per
                  wave instruction over 1024 SIMDs at 2.4 GHz
  graph_span_ms   the span of the whole graph
Needs the GPU; there is no fallback.
    python3 tools/brdf_lut_ggx_time.py [--out profiles/brdf_lut_ggx.json]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vulkan-pbr-renderer_amd", "python"))
import numpy as np  # noqa: E402
import pbrhip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "brdf_lut_ggx.json"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--size", type=int, default=256)
args = ap.parse_args()

VALU = {0: 29, 1: 48}
TERM = {0: "smith_schlick", 1: "smith_correlated"}
SIMDS, HZ = 1024, 2.4e9
COUNTS = (64, 1024, 4096)
n = args.size

L = pbrhip.init(0)
lut = pbrhip.make_texture(pbrhip.Format_RG16F, n, n, pbrhip.TextureFlag_StorageImage)
k1 = pbrhip.make_texture(pbrhip.Format_RG16F, n, n, pbrhip.TextureFlag_StorageImage)
pipes, arena, g = L.PBR_MakeIBLPipelines(), L.GPU_MakeDescriptorArena(), L.GPU_MakeGraph()
maps = pbrhip.PBR_IBLMaps()
maps.brdf_lut = k1
unit = (pbrhip.PBR_WorkUnit * 1)()
unit[0].kind = pbrhip.Unit_BrdfLut
unit[0].row0, unit[0].row1, unit[0].face0, unit[0].face1 = 0, n, 0, 1

order = [(count, vis) for count in COUNTS for vis in (0, 1)]
times, spans = {}, []
L.GPUX_EnableOpTiming(1)
for rep in range(args.repeats + 1):
    for count, vis in order:
        L.GPUX_OpBrdfLutGGX(g, lut, count, vis, 0, n)
    L.PBR_RecordUnits(pipes, g, arena, None, C.byref(maps), unit, 1)
    L.GPU_GraphSubmit(g)
    L.GPU_GraphWait(g)
    L.GPU_ResetDescriptorArena(arena)
    names = [L.GPUX_GraphTimedOpName(g, i).decode() for i in range(L.GPUX_GraphTimedOpCount(g))]
    assert names == ["K22.brdf_lut_ggx"] * len(order) + ["K1.brdf_lut"], names
    if rep == 0:
        continue                                                               # the first submission loads the code objects
    spans.append(L.GPUX_GraphSpanMs(g))
    for i, key in enumerate(order + ["k1"]):
        times.setdefault(key, []).append(L.GPUX_GraphTimedOpMs(g, i))
L.GPUX_EnableOpTiming(0)

out = {"what": f"K22 on a {n} x {n} RG16F map, N = {list(COUNTS)}, both visibility terms, and K1's {n} x {n} map at 4096 samples, one graph, one stream",
       "valu_per_sample": {TERM[v]: VALU[v] for v in VALU}, "repeats": args.repeats, "graph_span_ms": round(float(np.median(spans)), 4), "ops": []}
for count, vis in order:
    ms = float(np.median(times[(count, vis)]))
    floor_ms = n * n / 64 * count * VALU[vis] * 4 / (SIMDS * HZ) * 1e3
    out["ops"].append({"kernel": "K22.brdf_lut_ggx", "visibility": TERM[vis], "samples": count, "ms": round(ms, 5),
                       "ms_runs": [round(x, 5) for x in times[(count, vis)]], "ps_per_texel_sample": round(ms * 1e9 / (n * n * count), 3),
                       "valu_issue_floor_ms": round(floor_ms, 5), "fraction_of_valu_floor": round(floor_ms / ms, 3)})
ms = float(np.median(times["k1"]))
out["ops"].append({"kernel": "K1.brdf_lut", "samples": 4096, "ms": round(ms, 5), "ms_runs": [round(x, 5) for x in times["k1"]],
                   "ps_per_texel_sample": round(ms * 1e9 / (n * n * 4096), 3)})

print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
L.GPU_DestroyGraph(g); L.GPU_DestroyDescriptorArena(arena); L.PBR_DestroyIBLPipelines(pipes)
L.GPU_DestroyTexture(lut); L.GPU_DestroyTexture(k1)
L.GPU_WaitUntilIdle(); L.GPU_Deinit()
