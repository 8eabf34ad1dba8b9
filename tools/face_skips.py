#!/usr/bin/env python3
"""Absorbed-word counters of the region kernel (k_mc_region.hip, 2c) per FACE: every face of a C4 level dispatched alone under
PBR_MC_STATS=1, then the whole level.  One line per dispatch: absorbed wave-words, their wave-samples over the wave-samples the
tile's region passes visit (the skip fraction), count-only samples, healed wave-slices, and the time of the dispatch WITH the
counters on (tools/face_time.py gives times without them).  profiles/r06_order.md was made with this.
   python3 tools/face_skips.py [mip ...]"""
import ctypes as C
import os
import sys
import time

os.environ["PBR_MC_STATS"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "vulkan-pbr-renderer_amd", "python"))
import bench  # noqa: E402
import pbrhip  # noqa: E402
from pbrhip import mc  # noqa: E402

W, spec_size, irr_size, seed, _ = bench.WORKLOADS["c4"]
env = bench.load_env(W, seed, workers=6)
L = pbrhip.init()
env_tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, W, W, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
maps = pbrhip.PBR_IBLMaps(); L.PBR_MakeIBLMaps(C.byref(maps), 8, 64, spec_size)
pipes = L.PBR_MakeIBLPipelines(); arena = L.GPU_MakeDescriptorArena(); graph = L.GPU_MakeGraph()


def run(mip, f0, f1):
    u = (pbrhip.PBR_WorkUnit * 1)(pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, mip, f0, f1, 0, spec_size >> mip, 0.0))
    L.PBR_RecordUnits(pipes, graph, arena, env_tex, C.byref(maps), u, 1)
    L.GPU_WaitUntilIdle(); t0 = time.perf_counter()
    L.GPU_GraphSubmit(graph); L.GPU_GraphWait(graph)
    dt = (time.perf_counter() - t0) * 1e3
    L.GPU_ResetDescriptorArena(arena)
    return dt


run(2, 0, 1)                                   # the counters exist after the kernel's first launch
for mip in [int(a) for a in sys.argv[1:]] or [2, 1]:
    for f0, f1 in [(f, f + 1) for f in range(6)] + [(0, 6)]:
        mc.reset_counters(L)
        run(mip, f0, f1)
        c = mc.counters(L, "region", "skip", "flag")
        ms = min(run(mip, f0, f1) for _ in range(3))
        visited = 4 * c["flags"]               # four waves run every flagged (region, sample) of a tile
        print(f"mip {mip} faces [{f0}, {f1}): {c['abs_words']} wave-words absorbed, {c['abs_samples']} of {visited} wave-samples "
              f"({c['abs_samples'] / max(visited, 1):.3f}), {c['count_only']} count-only, {c['healed']} of {c['slices']} wave-slices healed, {ms:.3f} ms", flush=True)
L.GPU_WaitUntilIdle(); L.GPU_Deinit()
