#!/usr/bin/env python3
"""K12 (the sun depth pass) at the reference's 2048^2 over a ~1M-triangle synth_mesh_temple (~100 parts, one draw per part):
per-op times of K12.setup / K12.tiles (GPUX_EnableOpTiming, median of 20 passes) and the wall time per pass of 50 passes recorded
back to back into one graph (timing off), with Mtriangles/s and the fraction of 8 TB/s that the pass's algorithmic bytes (indices,
positions, the map read and written) represent.   python3 tools/sun_depth_time.py [--out profiles/sun_depth_1m.json]"""
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
from pbrhip import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sun_depth_1m.json"))
ap.add_argument("--triangles", type=int, default=1000000)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--passes", type=int, default=50)
ap.add_argument("--timed", type=int, default=20, help="passes timed with GPUX_EnableOpTiming")
ap.add_argument("--walls", type=int, default=5, help="repetitions of the back-to-back wall-time graph")
args = ap.parse_args()

verts, idx, parts = synth.synth_mesh_temple(args.triangles)
tris = len(idx) // 3
L = pbrhip.init(0)
sp = L.PBR_MakeSunDepthPass(args.size)
mesh = pbrhip.make_mesh(verts, idx, parts)
glob = pbrhip.fill_globals((0.0, -30.0, 6.0))
g = L.GPU_MakeGraph()

L.GPUX_EnableOpTiming(1)
per_op = {"K12.setup": [], "K12.tiles": []}
for it in range(args.timed + 2):
    L.PBR_RecordSunDepthPass(sp, g, mesh, C.byref(glob))
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    if it >= 2:
        for i in range(L.GPUX_GraphTimedOpCount(g)):
            name = L.GPUX_GraphTimedOpName(g, i).decode()
            if name in per_op:
                per_op[name].append(L.GPUX_GraphTimedOpMs(g, i))
L.GPUX_EnableOpTiming(0)

walls = []
for rep in range(args.walls):
    for _ in range(args.passes):
        L.PBR_RecordSunDepthPass(sp, g, mesh, C.byref(glob))
    t0 = time.perf_counter()
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    walls.append((time.perf_counter() - t0) / args.passes * 1e3)
cover = float((pbrhip.read_mip(L.PBR_SunDepthTexture(sp), 0)[..., 0] < 1).mean())

setup = float(np.median(per_op["K12.setup"])); tiles = float(np.median(per_op["K12.tiles"]))
wall = float(np.median(walls))
used_vertices = len(np.unique(idx))
algo_bytes = len(idx) * 4 + used_vertices * 12 + 2 * 4 * args.size * args.size
res = {
    "what": f"K12 sun depth pass, {args.size}^2 D32F, synth_mesh_temple({args.triangles}): {tris} triangles, {len(parts)} parts (one GPU_OpDrawIndexed each)",
    "triangles": tris, "parts": len(parts), "vertices": len(verts), "map_covered_fraction": round(cover, 4),
    "K12.setup_ms_median": round(setup, 4), "K12.tiles_ms_median": round(tiles, 4),
    "K12.setup_ms_all": [round(x, 4) for x in per_op["K12.setup"]], "K12.tiles_ms_all": [round(x, 4) for x in per_op["K12.tiles"]],
    "wall_ms_per_pass_median": round(wall, 4), "wall_ms_per_pass_runs": [round(x, 4) for x in walls],
    "passes_per_graph": args.passes,
    "mtriangles_per_s": round(tris / (wall * 1e-3) / 1e6, 1),
    "algorithmic_bytes": algo_bytes,
    "fraction_of_8TBps": round(algo_bytes / (wall * 1e-3) / 8e12, 4),
    "hbm_floor_us": round(algo_bytes / 8e12 * 1e6, 2),
}
print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
L.GPU_DestroyGraph(g); L.PBR_DestroyMesh(mesh); L.PBR_DestroySunDepthPass(sp)
L.GPU_WaitUntilIdle(); L.GPU_Deinit()
