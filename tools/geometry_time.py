#!/usr/bin/env python3
"""K13 (the geometry pass) at 1920 x 1080 over a ~1M-triangle synth_mesh_temple (~100 parts, one draw per part) with 16 materials of
256^2: per-op times of K13.setup / K13.tiles (GPUX_EnableOpTiming, median of the timed passes) and the busy span per pass
(GPUX_GraphSpanMs) of 20 passes recorded back to back into one graph, median of 5 graphs.  K12's time for the same mesh is read
from profiles/sun_depth_1m.json and recorded beside it as context.   python3 tools/geometry_time.py [--out profiles/geometry_1m.json]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vulkan-pbr-renderer_amd", "python"))
import numpy as np  # noqa: E402
import pbrhip  # noqa: E402
from pbrhip import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_1m.json"))
ap.add_argument("--triangles", type=int, default=1000000)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--materials", type=int, default=16)
ap.add_argument("--texture", type=int, default=256)
ap.add_argument("--passes", type=int, default=20)
ap.add_argument("--graphs", type=int, default=5)
ap.add_argument("--timed", type=int, default=5, help="passes timed with GPUX_EnableOpTiming")
args = ap.parse_args()

W, H = args.width, args.height
verts, idx, parts, part_mat = synth.synth_mesh_temple(args.triangles, n_materials=args.materials)
tris = len(idx) // 3
L = pbrhip.init(0)
gb = pbrhip.PBR_GBuffer()
L.PBR_MakeGBuffer(C.byref(gb), W, H, pbrhip.Format_RGBA16F)
pp = L.PBR_MakePostProcess(C.byref(gb), W, H, pbrhip.Format_RGBA8UN)
gp = L.PBR_MakeGeometryPass(C.byref(gb), pp, W, H)
materials = [pbrhip.make_material(m) for m in synth.synth_materials(args.materials, args.texture)]
mesh = pbrhip.make_mesh(verts, idx, parts)
for k, m in enumerate(part_mat):
    L.PBR_MeshSetPartMaterial(mesh, k, materials[m])
glob = pbrhip.fill_globals((0.0, -30.0, 6.0), aspect=W / H)
for k in range(16):
    glob.old_clip_space_from_world[k] = glob.clip_space_from_world[k]
g = L.GPU_MakeGraph()

L.GPUX_EnableOpTiming(1)
per_op = {"K13.setup": [], "K13.tiles": []}
for it in range(args.timed + 2):
    L.PBR_RecordGeometryPass(gp, g, mesh, None, C.byref(glob), None, None, 0)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    if it >= 2:
        for i in range(L.GPUX_GraphTimedOpCount(g)):
            name = L.GPUX_GraphTimedOpName(g, i).decode()
            if name in per_op:
                per_op[name].append(L.GPUX_GraphTimedOpMs(g, i))

spans = []                                                                 # the span is recorded only while op timing is on
for rep in range(args.graphs):
    for _ in range(args.passes):
        L.PBR_RecordGeometryPass(gp, g, mesh, None, C.byref(glob), None, None, 0)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    spans.append(L.GPUX_GraphSpanMs(g) / args.passes)
L.GPUX_EnableOpTiming(0)
cover = float((pbrhip.read_mip(gb.depth, 0)[..., 0] < 1).mean())

setup, tiles, span = float(np.median(per_op["K13.setup"])), float(np.median(per_op["K13.tiles"])), float(np.median(spans))
used_vertices = len(np.unique(idx))
algo_bytes = len(idx) * 4 + used_vertices * 44 + int(cover * W * H) * 28 + 4 * W * H + args.materials * 4 * (args.texture ** 2 * 4 * 4 // 3)
k12 = None
try:
    with open(os.path.join(ROOT, "profiles", "sun_depth_1m.json")) as f:
        k12 = json.load(f).get("wall_ms_per_pass_median")
except OSError:
    pass
res = {
    "what": f"K13 geometry pass, {W}x{H}, synth_mesh_temple({args.triangles}): {tris} triangles, {len(parts)} parts (one GPU_OpDrawIndexed each), "
            f"{args.materials} materials of {args.texture}^2",
    "triangles": tris, "parts": len(parts), "vertices": len(verts), "frame_covered_fraction": round(cover, 4),
    "K13.setup_ms_median": round(setup, 4), "K13.tiles_ms_median": round(tiles, 4),
    "span_ms_per_pass_median": round(span, 4), "span_ms_per_pass_graphs": [round(x, 4) for x in spans], "passes_per_graph": args.passes,
    "mtriangles_per_s": round(tris / (span * 1e-3) / 1e6, 1),
    "algorithmic_bytes": algo_bytes, "hbm_floor_us": round(algo_bytes / 8e12 * 1e6, 2),
    "context_K12_sun_depth_same_mesh_ms_per_pass": k12,
}
print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
L.GPU_DestroyGraph(g); L.PBR_DestroyMesh(mesh); L.PBR_DestroyGeometryPass(gp)
for m in materials:
    L.PBR_DestroyMaterial(m)
L.PBR_DestroyPostProcess(pp); L.PBR_DestroyGBuffer(C.byref(gb))
L.GPU_WaitUntilIdle(); L.GPU_Deinit()
