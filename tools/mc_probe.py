#!/usr/bin/env python3
"""Time pbrk_mc_filter (K4b) on synthetic levels: picoseconds per sample evaluation and clocks per wave-sample per CU for a
given (n_src, out_size, roughness).  Kernel choice follows the library (env PBR_MC_LDS / PBR_MC_REGION / PBR_MC_BINNED); env
PBR_MC_TILE32 = -1 | 0 | 1 goes to pbrk_mc_set_tile32 (the region kernel's 32 x 32 tile: by rule, never, wherever the shape allows);
PBR_MC_NET = -1 | 0 | 1 goes to pbrk_mc_set_net (the region kernel's completeness net: by rule, off where it can be, always on);
PBR_MC_RESIDENT=0 keeps levels of at most 16^2 texels off k_mc_resident (the library reads it).  The table is registered
(pbrk_mc_table_register), so the bin cache serves it by its default rule: the untimed first launch records, the timed ones replay;
PBR_MC_BIN_CACHE=0 keeps it off, PBR_MC_EXACT_BINS=0 keeps the recorded flags the bound's (the library reads both).
   python3 tools/mc_probe.py n_src out_size [roughness] [rows] [face0 face1]"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vulkan-pbr-renderer_amd", "python"))
import pbrhip  # noqa: E402
from pbrhip import mc  # noqa: E402
if os.environ.get("PBRHIP_LIB"):
    pbrhip.LIB_PATH = os.environ["PBRHIP_LIB"]


def main():
    n_src, out = int(sys.argv[1]), int(sys.argv[2])
    rough = float(sys.argv[3]) if len(sys.argv) > 3 else 0.15
    rows = int(sys.argv[4]) if len(sys.argv) > 4 else out
    f0, f1 = (int(sys.argv[5]), int(sys.argv[6])) if len(sys.argv) > 6 else (0, 6)
    L = pbrhip.init(0)
    if os.environ.get("PBR_MC_TILE32"):
        L.pbrk_mc_set_tile32(int(os.environ["PBR_MC_TILE32"]))
    if os.environ.get("PBR_MC_NET"):
        L.pbrk_mc_set_net(int(os.environ["PBR_MC_NET"]))
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    lvl = rng.random((6, n_src, n_src, 4), dtype=np.float32) + 0.1
    pyr = torch.from_numpy(lvl).to(dev)
    bord = torch.zeros((6, n_src + 2, n_src + 2, 4), dtype=torch.float32, device=dev)
    assert L.pbrk_border_build(pyr.data_ptr(), bord.data_ptr(), n_src, 1, None) == 0
    cells = torch.zeros(L.pbrk_cells_bytes(n_src) // 4, dtype=torch.float32, device=dev)
    use_cells = n_src <= 512
    if use_cells:
        assert L.pbrk_cells_build(bord.data_ptr(), n_src, cells.data_ptr(), None) == 0
    tab = np.zeros((8192, 4), dtype=np.float32)
    alpha = C.c_float()
    n_tab = L.pbrk_host_prefilter_table(8192, rough, tab.ctypes.data_as(C.c_void_p), C.byref(alpha))
    dtab = torch.from_numpy(tab).to(dev)
    assert L.pbrk_mc_table_register(dtab.data_ptr(), n_tab) == 0
    outt = torch.zeros((6, out, out, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def run():
        rc = L.pbrk_mc_filter(bord.data_ptr(), cells.data_ptr() if use_cells else None, n_src, dtab.data_ptr(), n_tab,
                              float(np.pi), alpha.value, outt.data_ptr(), out, f0, f1, 0, rows, None)
        assert rc == 0, rc

    run(); torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); run(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ms = min(ts)
    evals = float(f1 - f0) * out * rows * n_tab
    ps = ms * 1e-3 / evals * 1e12
    clk = ps * 1e-12 * 256 * 2.4e9 * 64
    chk = float(outt[:, :rows].double().sum().item())
    print(f"n_src {n_src} out {out} rows {rows} faces {f0}-{f1} n_tab {n_tab}: {ms:.3f} ms  {ps:.3f} ps/eval  {clk:.1f} clk per wave-sample per CU @2.4GHz  "
          f"{65 * evals / ms * 1e-9:.1f} TFLOP/s alg  checksum {chk:.6e}", flush=True)
    if os.environ.get("PBR_MC_STATS") == "1":
        rs = (C.c_uint64 * 4)()                                # k_mc_resident's own counters: read ahead of the reset below
        if L.pbrk_mc_resident_stats(rs) == 0 and rs[2] + rs[3]:
            pairs = rs[2] + rs[3]
            print(f"   resident kernel: {rs[2] / pairs:.3f} of the (texel, sample) pairs taken by proved runs, {rs[3] / pairs:.3f} by the general pass, "
                  f"{rs[1]} proved (tile, sample) pairs, {rs[0]} proof violations", flush=True)
        c = mc.counters(L, "flag", "window", "skip", "cut", "phase", "region", reset=True, missing_ok=True)
        if c.get("flag_samples"):
            tiles = c["flag_samples"] // n_tab
            print(f"   binning: {c['flags'] / c['flag_samples']:.3f} regions flagged per sample, {c['visits'] / tiles:.2f} regions visited per tile ({tiles} tile launches), "
                  f"{c.get('proved', 0) / c['flag_samples']:.3f} of the samples proved in-region for the whole tile (test-free body)", flush=True)
        if "abs_samples" in c and "cut4" in c and c.get("flags"):
            print(f"   absorbed: {c['abs_samples'] / (4 * c['flags']):.4f} of the flagged wave-samples ({c['count_only']} through the count-only body); cut words {c['cut4']} of {c['nw']}, "
                  f"{c['words_cut']} words cut", flush=True)
        if c.get("phase", (0, 0))[1] and c.get("slices"):
            tiles = c["slices"] // 16                          # workgroups: sixteen waves each (the flag counters count blocks of 256 texels)
            print("   clocks per tile (frames, clearing + binning, staging, region passes, reduction + store): "
                  + ", ".join(f"{v / tiles:.0f}" for v in c["phase"]), flush=True)
        if "healed" in c:
            print(f"   region kernel: {c['healed']} of {c['slices']} wave-slices recomputed with direct loads", flush=True)
    bc = mc.bin_cache_stats(L)
    print(f"   bin cache: {bc['recorded']} recording, {bc['replayed']} replaying, {bc['computed']} computing launches, {bc['bytes']} bytes held", flush=True)
    if hasattr(mc, "exact_bins_stats"):
        xb = mc.exact_bins_stats(L)
        if xb["flags_before"]:
            print(f"   exact bins (summed over the tiles of the recorded entry, {n_tab} samples each): flags {xb['flags_before']} -> {xb['flags_after']}, "
                  f"proved {xb['proved_before']} -> {xb['proved_after']}, stagings asked for {xb['any_before']} -> {xb['any_after']}, "
                  f"unset hits {xb['unset_hits']}, lost lanes {xb['lost_lanes']}", flush=True)
    L.GPU_WaitUntilIdle(); L.pbrk_mc_table_unregister(dtab.data_ptr()); L.GPU_Deinit()


if __name__ == "__main__":
    main()
