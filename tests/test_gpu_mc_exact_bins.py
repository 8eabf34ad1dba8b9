"""Exact flags in the bin cache (k_mc_region.hip, header 2n; pbrk_mc_set_exact_bins): behind a recording launch k_mc_refine_bins rewrites
the entry so that a flag stays exactly where some lane of the tile takes the sample and a proof bit is set exactly where all lanes take it
in one region.  A replay of refined words accumulates the pairs the bound's words accumulate, in the same order: every byte must equal
the replay of unrefined words and the run with the cache off.  A missing flag or a wrong proof would move a tap.

The suite runs with the device counters on, where the default rules keep the cache and the refinement off: both are asked for by name,
and the rule is checked in child processes.  256^2 outputs (264^2 for clipped tiles); tables of roughness 0.03 (1389 samples: launch cut,
absorbed words) and 0.15 (8192), each whole, its first 1000 samples and its first 100, as in test_gpu_mc_bin_cache.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mc_cases import OUT, WINDOWS, level
from pbrhip import mc

pytestmark = pytest.mark.gpu

# (n_src, tile32, output size): quarter faces with both tiles, whole faces, clipped tiles, no fold (48, 24), the 34^2 shape
SHAPES = [(128, 0, 256), (128, 1, 256), (64, 0, 256), (64, 0, 264), (48, 0, 256), (24, 0, 256), (32, 0, 256)]
ROUGHS = [0.03, 0.15]
TABLES = [None, 1000, 100]
SINGLE_FACES = [(f, f + 1, 0, OUT) for f in range(6)]


@pytest.fixture(scope="module")
def tables(gpu):
    L = gpu
    for rough in ROUGHS:
        dtab, n_full, _ = mc.prefilter_table(L, rough)
        assert n_full > 1000 and L.pbrk_mc_table_register(dtab.ptr, n_full) == 0
    yield
    L.pbrk_mc_bin_cache_clear()
    for rough in ROUGHS:
        assert L.pbrk_mc_table_unregister(mc.prefilter_table(L, rough)[0].ptr) == 0


@pytest.fixture(autouse=True)
def fresh_cache(gpu):
    gpu.pbrk_mc_bin_cache_clear()
    mc.exact_bins_stats(gpu, reset=True)
    yield
    gpu.pbrk_mc_bin_cache_clear()


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"n{s[0]}t{s[1]}o{s[2]}")
def shape(request, gpu, tables):
    n_src, tile32, out = request.param
    bord = mc.BorderedLevel(gpu, level(n_src))
    yield n_src, tile32, out, bord
    bord.free()


def _run(L, bord, rough, n_tab, tile32, cache, exact, windows=None, out=OUT, net=-1):
    """One dispatch set into a cleared cube: (bytes, region counters, what the cache's counters moved by, pbrk_mc_last_exact_bins)."""
    windows = windows or [(0, 6, 0, out)]
    with mc.switches(L, tile32=tile32, bin_cache=cache, exact_bins=exact, net=net):
        mc.reset_counters(L)
        before = mc.bin_cache_stats(L)
        data = mc.filter_windows(L, bord, rough, windows, out, n_tab)
        after = mc.bin_cache_stats(L)
        c = mc.counters(L, "flag", "window", "region", reset=True)
        return data, c, {k: after[k] - before[k] for k in mc.BIN_CACHE_KEYS[:4]}, L.pbrk_mc_last_exact_bins()


def _region_kernel_serves(L, n_src, rough, n_tab):
    # 24 quarter-face regions x 256 mask words do not fit the region kernel's LDS: another kernel serves the level, nothing is recorded
    return not (n_src > 64 and (n_tab or mc.prefilter_table(L, rough)[1]) == 8192)


@pytest.mark.parametrize("n_tab", TABLES, ids=lambda n: f"tab{n or 'full'}")
@pytest.mark.parametrize("rough", ROUGHS, ids=lambda r: f"r{r}")
def test_bytes_against_unrefined_replay(gpu, shape, rough, n_tab):
    L = gpu
    n_src, tile32, out, bord = shape
    tag = f"n_src {n_src} tile32 {tile32} out {out} rough {rough} n_tab {n_tab or 'full'}"
    off = _run(L, bord, rough, n_tab, tile32, 0, 0, out=out)
    rec0 = _run(L, bord, rough, n_tab, tile32, 1, 0, out=out)
    rep0 = _run(L, bord, rough, n_tab, tile32, 1, 0, out=out)
    L.pbrk_mc_bin_cache_clear()
    rec1 = _run(L, bord, rough, n_tab, tile32, 1, 1, out=out)
    rep1 = _run(L, bord, rough, n_tab, tile32, 1, 1, out=out)
    st = mc.exact_bins_stats(L)
    print(f"{tag}: bound {rep0[1]}; refined {rep1[1]}; {st}")
    for name, run in (("recording, bound", rec0), ("replay, bound", rep0), ("recording, refined behind it", rec1), ("replay, refined", rep1)):
        assert run[1]["healed"] == 0, (tag, name, run[1])
        assert run[0] == off[0], f"{tag}: {name}: the bytes moved"
    if not _region_kernel_serves(L, n_src, rough, n_tab):
        assert rec1[2]["recorded"] == 0 and st["flags_before"] == 0, (tag, rec1[2], st)
        return
    assert all(run[1]["slices"] > 0 for run in (rec0, rep0, rec1, rep1)), tag
    assert rec0[2]["recorded"] == 1 and rep0[2]["replayed"] == 1 and rec0[3] == 0, (tag, rec0[2], rep0[2], rec0[3])
    assert rec1[2]["recorded"] == 1 and rep1[2]["replayed"] == 1 and rec1[3] == 1, (tag, rec1[2], rep1[2], rec1[3])
    # the recording launch ran on the bound's flags, the replay on the refined ones: what the counters saw of them
    assert rec1[1]["flags"] == rec0[1]["flags"] == rep0[1]["flags"] and rep1[1]["flags"] <= rep0[1]["flags"], (tag, rec1[1], rep1[1])
    assert st["flags_before"] > 0 and st["unset_hits"] == 0 and st["lost_lanes"] == 0, (tag, st)


@pytest.mark.parametrize("n_tab", TABLES, ids=lambda n: f"tab{n or 'full'}")
@pytest.mark.parametrize("rough", ROUGHS, ids=lambda r: f"r{r}")
def test_completeness_under_the_net(gpu, shape, rough, n_tab):
    """Counters on, net on: a refined replay heals no wave-slice; flags fall, proofs rise, the bound was never exceeded."""
    L = gpu
    n_src, tile32, out, bord = shape
    if not _region_kernel_serves(L, n_src, rough, n_tab):
        return
    tag = f"n_src {n_src} tile32 {tile32} out {out} rough {rough} n_tab {n_tab or 'full'}"
    rec = _run(L, bord, rough, n_tab, tile32, 1, 1, out=out, net=1)
    assert L.pbrk_mc_last_net() == 1
    rep = _run(L, bord, rough, n_tab, tile32, 1, 1, out=out, net=1)
    assert L.pbrk_mc_last_net() == 1
    st = mc.exact_bins_stats(L)
    print(f"{tag}: recording {rec[1]}; replay {rep[1]}; {st}")
    assert rec[2]["recorded"] == 1 and rep[2]["replayed"] == 1 and rec[3] == 1, (tag, rec[2], rep[2])
    assert rec[1]["healed"] == 0 and rep[1]["healed"] == 0 and rep[1]["slices"] == rec[1]["slices"] > 0, (tag, rec[1], rep[1])
    assert st["flags_after"] <= st["flags_before"] and st["proved_after"] >= st["proved_before"], (tag, st)
    assert st["any_after"] <= st["any_before"], (tag, st)
    assert st["unset_hits"] == 0 and st["lost_lanes"] == 0, (tag, st)
    if (n_src, out) in ((32, 256), (64, 256)):
        assert st["flags_after"] < st["flags_before"], (tag, st)


def _rows(data, out, window):
    f0, f1, y0, rows = window
    return np.frombuffer(data, np.float32).reshape(6, out, out, 4)[f0:f1, y0:y0 + rows].tobytes()


@pytest.mark.parametrize("n_src,tile32", [(128, 0), (128, 1), (64, 0), (32, 0)], ids=lambda v: str(v))
def test_windows(gpu, tables, n_src, tile32):
    """The pole rows of +-X, a ragged window and single faces under a refined entry: eligible windows replay the refined words, the others
    bin as ever; each window's rows are the full dispatch's."""
    L = gpu
    tile = 32 if tile32 else 16
    bord = mc.BorderedLevel(L, level(n_src))
    try:
        off = _run(L, bord, 0.03, None, tile32, 0, 0)
        rec = _run(L, bord, 0.03, None, tile32, 1, 1)
        assert rec[2]["recorded"] == 1 and rec[3] == 1 and rec[0] == off[0], rec[2]
        for windows in (WINDOWS, SINGLE_FACES):
            eligible = sum(L.pbrk_mc_bin_window_eligible(OUT, tile, y0, y0 + rows) for _, _, y0, rows in windows)
            got = _run(L, bord, 0.03, None, tile32, 1, 1, windows)
            assert (got[2]["replayed"], got[2]["computed"], got[2]["recorded"]) == (eligible, len(windows) - eligible, 0), (windows, got[2])
            assert got[1]["healed"] == 0
            for w in windows:
                assert _rows(got[0], OUT, w) == _rows(off[0], OUT, w), w
        assert sum(L.pbrk_mc_bin_window_eligible(OUT, tile, y0, y0 + rows) for _, _, y0, rows in WINDOWS) == (0 if tile32 else 2)
    finally:
        bord.free()


@pytest.mark.parametrize("n_src,tile32", [(128, 0), (128, 1), (64, 0)], ids=lambda v: str(v))
def test_the_cut_moves_under_refined_words(gpu, tables, n_src, tile32):
    """The entry holds every sample's refined flags; the launch cut moves with the level's texels.  Recorded and refined on the stock
    level, replayed on the level with a 4 x 4 patch scaled by 1e5, then on a level of ones: each equals its own run with the cache off."""
    L = gpu
    stock = level(128)
    bright = stock.copy()
    bright[4, 58:62, 58:62, :3] *= 1e5
    crop = lambda lvl: np.ascontiguousarray(lvl[:, :n_src, :n_src])
    bord = mc.BorderedLevel(L, crop(stock))
    try:
        rec = _run(L, bord, 0.03, None, tile32, 1, 1)
        cut_rec = mc.counters(L, "cut")
        assert rec[2]["recorded"] == 1 and rec[3] == 1, rec[2]
    finally:
        bord.free()
    for name, lvl in (("bright", bright), ("ones", np.ones_like(stock))):
        bord = mc.BorderedLevel(L, crop(lvl))
        try:
            rep = _run(L, bord, 0.03, None, tile32, 1, 1)
            cut_rep = mc.counters(L, "cut")
            off = _run(L, bord, 0.03, None, tile32, 0, 0)
        finally:
            bord.free()
        print(f"n_src {n_src} tile32 {tile32} {name}: cut {cut_rep} (recorded at {cut_rec}); {rep[1]}")
        assert rep[2]["replayed"] == 1 and rep[2]["recorded"] == 0, (name, rep[2])
        assert rep[1]["healed"] == 0 and off[1]["healed"] == 0 and rep[0] == off[0], f"{name}: the bytes moved"
        if name == "bright":
            assert cut_rec["words_cut"] > 0 and cut_rep["cut4"] != cut_rec["cut4"], (cut_rec, cut_rep)


def _child(stats_env):
    env = dict(os.environ)
    for k in ("PBR_MC_STATS", "PBR_MC_BIN_CACHE", "PBR_MC_EXACT_BINS"):
        env.pop(k, None)
    if stats_env is not None:
        env["PBR_MC_STATS"] = stats_env
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mc_exact_bins_child.py")
    done = subprocess.run([sys.executable, script], env=env, capture_output=True, text=True, timeout=180)
    assert done.returncode == 0, done.stderr[-2000:]
    return json.loads(done.stdout.strip().splitlines()[-1])


def test_default_rule_counters_off(gpu):
    """A fresh process without PBR_MC_STATS, mode -1: the recording launch of a shape the host rule takes (34^2: n_src 32) is followed
    by the refinement, that of a shape it leaves out (66^2 whole faces: n_src 64) is not; same bytes."""
    res = _child(None)
    print(res)
    assert res["stats_env"] is None
    for n_src, r in res["levels"].items():
        assert r["last_exact"] == (1 if n_src == "32" else 0) and r["moved"] == [1, 2], (n_src, r)
        assert r["on"] == [r["off"]] * 3, n_src
    e = res["exact"]
    assert e["flags_before"] > e["flags_after"] > 0 and e["unset_hits"] == 0 and e["lost_lanes"] == 0, e


def test_default_rule_counters_on(gpu):
    """The same with PBR_MC_STATS=1: the cache, asked for by name, records; the rule keeps the refinement off."""
    res = _child("1")
    print(res)
    assert res["stats_env"] == "1"
    for n_src, r in res["levels"].items():
        assert r["last_exact"] == 0 and r["moved"] == [1, 2], (n_src, r)
        assert r["on"] == [r["off"]] * 3, n_src
    assert res["exact"]["flags_before"] == 0, res["exact"]
