"""The bin cache of the region and resident kernels (k_mc_region.hip, header 2m; pbrk_mc_set_bin_cache): the first whole-level launch of a
(kernel shape, level shape, registered table) stores every tile's binning flags, every later eligible launch copies them instead of
computing them.  The samples taken, their order and the absorb decisions do not change, so a replaying launch must give the bytes and
the counters of a computing one on every shape that takes part: quarter faces with both tiles, whole faces folded and unfolded, the 34^2
shape, the resident kernel with both tiles and both folds, an output whose last tile row and column are clipped.

The suite runs with the device counters on, where the default rule (-1) keeps the cache off: the states are asked for by name here, and
the rule itself is checked in child processes.  256^2 outputs (128^2 for the 8 x 8 tile of the resident kernel).  Tables: roughness
0.03 (1389 samples: the launch cut, absorbed words) and 0.15 (8192), each whole, its first 1000 samples and its first 100."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pbrhip
from mc_cases import OUT, level
from pbrhip import mc

pytestmark = pytest.mark.gpu

# (n_src, tile32, output size)
# 64 -> 250^2: the region kernel takes outputs of 256^2 and more, so another kernel serves this level and the cache has nothing to act on;
# the clipped last tile row and column it was meant for are met by 64 -> 264^2 (region kernel) and 16 -> 250^2 (resident kernel, 8 x 8 tiles)
SHAPES = [(128, 0, 256), (128, 1, 256), (64, 0, 256), (48, 0, 256), (32, 0, 256), (16, 0, 256), (12, 0, 256), (8, 0, 128), (64, 0, 250),
          (64, 0, 264), (16, 0, 250)]
ROUGHS = [0.03, 0.15]
TABLES = [None, 1000, 100]
# three shards per face at tile rows of both tiles, then every face on its own
TILE_SHARDS = [(f, f + 1, a, b - a) for f in range(6) for a, b in ((0, 64), (64, 160), (160, OUT))]
SINGLE_FACES = [(f, f + 1, 0, OUT) for f in range(6)]
# the ragged shards of test_gpu_mc_net.py: no cut is a multiple of 16
RAGGED = [(f, f + 1, a, b - a) for f in range(6) for a, b in ((0, 5 + f), (5 + f, 131 - 2 * f), (131 - 2 * f, OUT))]
DEFAULT_BUDGET = 512 << 20


@pytest.fixture(scope="module")
def tables(gpu):
    """The two reference tables, registered for this module."""
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
    yield
    gpu.pbrk_mc_bin_cache_clear()
    gpu.pbrk_mc_set_bin_cache_budget(DEFAULT_BUDGET)


def _resident_counters(L):
    buf = (C.c_uint64 * 4)()
    if L.pbrk_mc_resident_stats(buf) != 0:
        return {}
    return dict(zip(("violations", "res_proved", "res_runs", "res_general"), (int(v) for v in buf)))


def _run(L, bord, rough, n_tab, tile32, mode, windows=None, out=OUT):
    """One dispatch set (default: the whole level) into a cleared cube: (bytes, counters, what the cache's counters moved by, the launch cut)."""
    windows = windows or [(0, 6, 0, out)]
    with mc.switches(L, tile32=tile32, bin_cache=mode):
        mc.reset_counters(L)
        before = mc.bin_cache_stats(L)
        data = mc.filter_windows(L, bord, rough, windows, out, n_tab)
        after = mc.bin_cache_stats(L)
        cut = mc.counters(L, "cut")
        c = _resident_counters(L)
        c.update(mc.counters(L, "skip", "flag", "window", "region", reset=True, missing_ok=True))
        moved = {k: after[k] - before[k] for k in mc.BIN_CACHE_KEYS[:4]}
        moved["bytes"] = after["bytes"]
        return data, c, moved, cut


def _same(a, b, tag):
    assert a[1] == b[1], (tag, a[1], b[1])
    assert a[1].get("healed", 0) == 0 and a[1].get("violations", 0) == 0 and a[1].get("slices", 0) > 0, (tag, a[1])
    assert a[0] == b[0], f"{tag}: the bytes moved"


def _moved(run, recorded=0, replayed=0, computed=0, declined=0):
    m = run[2]
    return (m["recorded"], m["replayed"], m["computed"], m["declined"]) == (recorded, replayed, computed, declined)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"n{s[0]}t{s[1]}o{s[2]}")
def shape(request, gpu, tables):
    n_src, tile32, out = request.param
    bord = mc.BorderedLevel(gpu, level(n_src))
    yield n_src, tile32, out, bord
    bord.free()


@pytest.mark.parametrize("n_tab", TABLES, ids=lambda n: f"tab{n or 'full'}")
@pytest.mark.parametrize("rough", ROUGHS, ids=lambda r: f"r{r}")
def test_record_then_replay(gpu, shape, rough, n_tab):
    L = gpu
    n_src, tile32, out, bord = shape
    tag = f"n_src {n_src} tile32 {tile32} out {out} rough {rough} n_tab {n_tab or 'full'}"
    off = _run(L, bord, rough, n_tab, tile32, 0, out=out)
    rec = _run(L, bord, rough, n_tab, tile32, 1, out=out)
    rep = _run(L, bord, rough, n_tab, tile32, 1, out=out)
    print(f"{tag}: {off[1]}; record {rec[2]}; replay {rep[2]}")
    assert _moved(off), (tag, off[2])
    if (n_src > 64 and (n_tab or mc.prefilter_table(L, rough)[1]) == 8192) or (n_src > 16 and out < 256):
        # 24 quarter-face regions x 256 mask words do not fit the region kernel's LDS, and it takes no output below 256^2: another kernel
        # serves the level, the cache has nothing to act on.  The case stays: no entry, the same bytes.
        assert _moved(rec) and _moved(rep) and rec[2]["bytes"] == 0 and off[0] == rec[0] == rep[0], (tag, rec[2], rep[2])
        return
    assert _moved(rec, recorded=1) and rec[2]["bytes"] > 0, (tag, rec[2])
    assert _moved(rep, replayed=1) and rep[2]["bytes"] == rec[2]["bytes"], (tag, rep[2])
    _same(off, rec, tag + " (recording)")
    _same(off, rep, tag + " (replaying)")


@pytest.mark.parametrize("n_src,tile32", [(128, 0), (128, 1), (64, 0)], ids=lambda v: str(v))
def test_the_cut_moves_under_a_warm_cache(gpu, tables, n_src, tile32):
    """The entry holds the flags of every sample, because the launch cut depends on the level's texels: recorded on the stock level,
    replayed on (a) the level with a 4 x 4 patch scaled by 1e5 -- its maximum rises, the cut keeps more words -- and (b) a level of ones,
    which keeps fewer.  Each equals its own computing run.  Against a vacuous pass the cut of (a) must differ from the recording level's."""
    L = gpu
    stock = level(128)
    bright = stock.copy()
    bright[4, 58:62, 58:62, :3] *= 1e5
    ones = np.ones_like(stock)
    crop = lambda lvl: np.ascontiguousarray(lvl[:, :n_src, :n_src])
    bord = mc.BorderedLevel(L, crop(stock))
    try:
        rec = _run(L, bord, 0.03, None, tile32, 1)
        assert _moved(rec, recorded=1), rec[2]
    finally:
        bord.free()
    for name, lvl in (("bright", bright), ("ones", ones)):
        bord = mc.BorderedLevel(L, crop(lvl))
        try:
            rep = _run(L, bord, 0.03, None, tile32, 1)
            off = _run(L, bord, 0.03, None, tile32, 0)
        finally:
            bord.free()
        print(f"n_src {n_src} tile32 {tile32} {name}: cut {rep[3]} (recorded at {rec[3]}); {rep[1]}")
        assert _moved(rep, replayed=1) and _moved(off), (name, rep[2], off[2])
        assert rep[3] == off[3], (name, rep[3], off[3])
        _same(off, rep, f"n_src {n_src} tile32 {tile32} {name}")
        if name == "bright":
            assert rec[3]["words_cut"] > 0 and rep[3]["cut4"] != rec[3]["cut4"], (rec[3], rep[3])
        else:
            assert rep[3]["words_cut"] >= rec[3]["words_cut"], (rec[3], rep[3])


@pytest.mark.parametrize("n_src,tile32", [(128, 0), (128, 1), (64, 0), (32, 0), (16, 0)], ids=lambda v: str(v))
def test_windows(gpu, tables, n_src, tile32):
    """Shards that start at a tile row and single faces replay; ragged shards compute on the region kernel (its tiles start at the
    dispatch's first row) and replay on the resident kernel (its tiles are anchored at row 0 of the face).  All equal the full dispatch."""
    L = gpu
    bord = mc.BorderedLevel(L, level(n_src))
    try:
        off = _run(L, bord, 0.03, None, tile32, 0)
        # a window finds nothing to replay before a whole-level launch has recorded, and records nothing itself
        early = _run(L, bord, 0.03, None, tile32, 1, [TILE_SHARDS[4]])
        assert _moved(early, computed=1) and early[2]["bytes"] == 0, early[2]
        rec = _run(L, bord, 0.03, None, tile32, 1)
        assert _moved(rec, recorded=1) and rec[0] == off[0], rec[2]
        for name, windows in (("tile shards", TILE_SHARDS), ("faces", SINGLE_FACES)):
            got = _run(L, bord, 0.03, None, tile32, 1, windows)
            assert _moved(got, replayed=len(windows)), (name, got[2])
            assert got[1]["healed"] == 0 and got[0] == off[0], name
        got = _run(L, bord, 0.03, None, tile32, 1, RAGGED)
        if n_src <= 16:
            assert _moved(got, replayed=len(RAGGED)), got[2]
        else:
            assert _moved(got, computed=len(RAGGED)), got[2]
        assert got[1]["healed"] == 0 and got[0] == off[0]
    finally:
        bord.free()


def _upload(L, dev, array):
    host = L.GPU_MakeBuffer(array.nbytes, pbrhip.BufferFlag_CPU, array.ctypes.data_as(C.c_void_p))
    g = L.GPU_MakeGraph()
    try:
        L.GPU_WaitUntilIdle()
        L.GPU_OpCopyBufferToBuffer(g, host, dev.buf, 0, 0, array.nbytes); L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    finally:
        L.GPU_DestroyGraph(g)
        L.GPU_DestroyBuffer(host)


def _filter_own(L, bord, dtab, n_tab, alpha, mode):
    zero = np.zeros((6, OUT, OUT, 4), np.float32)
    out = mc.DeviceBuffer(L, zero.nbytes, zero)
    try:
        with mc.switches(L, bin_cache=mode):
            before = mc.bin_cache_stats(L)
            assert L.pbrk_mc_filter(bord.dev.ptr, None, bord.n_src, dtab.ptr, n_tab, float(np.pi), alpha, out.ptr, OUT, 0, 6, 0, OUT, None) == 0
            data = out.read()
            after = mc.bin_cache_stats(L)
            moved = {k: after[k] - before[k] for k in mc.BIN_CACHE_KEYS[:4]}
            moved["bytes"] = after["bytes"]
            return data, None, moved
    finally:
        out.free()


@pytest.mark.parametrize("n_src", [64, 16])
def test_tables(gpu, n_src):
    """An unregistered table never records; a table registered again is a new generation; a prefix of a registered table has its own entry."""
    L = gpu
    tab = np.zeros((8192, 4), dtype=np.float32)
    alpha = C.c_float()
    n = L.pbrk_host_prefilter_table(8192, 0.03, tab.ctypes.data_as(C.c_void_p), C.byref(alpha))
    tab = np.ascontiguousarray(tab[:n])
    dtab = mc.DeviceBuffer(L, tab.nbytes, tab)
    bord = mc.BorderedLevel(L, level(n_src))
    try:
        off = _filter_own(L, bord, dtab, n, alpha.value, 0)
        for _ in range(2):
            got = _filter_own(L, bord, dtab, n, alpha.value, 1)
            assert _moved(got, computed=1) and got[2]["bytes"] == 0 and got[0] == off[0], got[2]
        assert L.pbrk_mc_table_register(dtab.ptr, n) == 0
        rec = _filter_own(L, bord, dtab, n, alpha.value, 1)
        rep = _filter_own(L, bord, dtab, n, alpha.value, 1)
        assert _moved(rec, recorded=1) and _moved(rep, replayed=1) and rec[0] == off[0] == rep[0], (rec[2], rep[2])
        held = rep[2]["bytes"]
        # a prefix: its own entry beside the whole table's
        off1000 = _filter_own(L, bord, dtab, 1000, alpha.value, 0)
        rec1000 = _filter_own(L, bord, dtab, 1000, alpha.value, 1)
        rep1000 = _filter_own(L, bord, dtab, 1000, alpha.value, 1)
        assert _moved(rec1000, recorded=1) and _moved(rep1000, replayed=1) and held < rec1000[2]["bytes"] < 2 * held, (rec1000[2], held)
        assert rec1000[0] == off1000[0] == rep1000[0]            # (the launch cut may drop the tail anyway: these can be the whole table's bytes)
        # unregister, send samples 3 .. 40 to the opposite side in x (other faces, other flags), register again
        assert L.pbrk_mc_table_unregister(dtab.ptr) == 0
        assert mc.bin_cache_stats(L)["bytes"] == 0
        tab2 = tab.copy()
        tab2[3:40, 0] *= -1.0
        _upload(L, dtab, tab2)
        assert L.pbrk_mc_table_register(dtab.ptr, n) == 0
        off2 = _filter_own(L, bord, dtab, n, alpha.value, 0)
        rec2 = _filter_own(L, bord, dtab, n, alpha.value, 1)
        rep2 = _filter_own(L, bord, dtab, n, alpha.value, 1)
        assert off2[0] != off[0]
        assert _moved(rec2, recorded=1) and _moved(rep2, replayed=1) and rec2[2]["bytes"] == held, (rec2[2], rep2[2])
        assert rec2[0] == off2[0] == rep2[0]
    finally:
        L.pbrk_mc_table_unregister(dtab.ptr)
        bord.free()
        dtab.free()


def test_budget_and_clear(gpu, tables):
    L = gpu
    bord = mc.BorderedLevel(L, level(64))
    try:
        off = _run(L, bord, 0.03, None, 0, 0)
        L.pbrk_mc_set_bin_cache_budget(4096)                       # the entry: 6 x 16 x 16 tiles x 7 x 44 words
        for _ in range(2):
            got = _run(L, bord, 0.03, None, 0, 1)
            assert _moved(got, computed=1, declined=1) and got[2]["bytes"] == 0 and got[0] == off[0], got[2]
        L.pbrk_mc_set_bin_cache_budget(DEFAULT_BUDGET)
        rec = _run(L, bord, 0.03, None, 0, 1)
        assert _moved(rec, recorded=1) and rec[2]["bytes"] == 6 * 16 * 16 * 7 * 44 * 4 and rec[0] == off[0], rec[2]
        L.pbrk_mc_bin_cache_clear()
        assert mc.bin_cache_stats(L)["bytes"] == 0
        again = _run(L, bord, 0.03, None, 0, 1)
        rep = _run(L, bord, 0.03, None, 0, 1)
        assert _moved(again, recorded=1) and _moved(rep, replayed=1) and again[0] == off[0] == rep[0], (again[2], rep[2])
    finally:
        bord.free()


def test_two_streams(gpu, c4_env):
    """A 512^2 specular job from the C4 environment as whole-level work units through PBR_RecordUnits, the levels side by side on the
    job's streams as by default: recorded by the first job, replayed by the second -- on whichever stream a level lands, behind the
    recording launch's event.  Level digests of the job with the cache off."""
    L = gpu
    tex = mc.env_texture(c4_env)
    S, mips = 512, (1, 2, 3, 4, 5)
    units = [pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, m, 0, 6, 0, S >> m, 0.0) for m in mips]

    def job(mode):
        with mc.switches(L, bin_cache=mode):
            before = mc.bin_cache_stats(L)
            with mc.dispatch_prefilter_units(L, tex, S, units) as maps:
                c = mc.counters(L, "region", reset=True)
                assert c["healed"] == 0 and c["slices"] > 0, c
                after = mc.bin_cache_stats(L)
                return ({m: mc.digest(pbrhip.read_mip(maps.tex_specular_env_map, m)) for m in mips},
                        {k: after[k] - before[k] for k in mc.BIN_CACHE_KEYS[:4]})

    try:
        off, m0 = job(0)
        first, m1 = job(1)
        second, m2 = job(1)
    finally:
        L.GPU_DestroyTexture(tex)
    print(f"512^2 job: cache off {m0}; first {m1}; second {m2}")
    assert (m0["recorded"], m0["replayed"]) == (0, 0)
    assert m1["recorded"] >= 1 and m2["recorded"] == 0 and m2["replayed"] >= m1["recorded"], (m1, m2)
    assert first == off and second == off


def _child(stats_env):
    env = dict(os.environ)
    env.pop("PBR_MC_STATS", None)
    env.pop("PBR_MC_BIN_CACHE", None)
    if stats_env is not None:
        env["PBR_MC_STATS"] = stats_env
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mc_bin_cache_child.py")
    done = subprocess.run([sys.executable, script], env=env, capture_output=True, text=True, timeout=180)
    assert done.returncode == 0, done.stderr[-2000:]
    return json.loads(done.stdout.strip().splitlines()[-1])


def test_default_rule_counters_off(gpu):
    """A fresh process without PBR_MC_STATS, mode -1: the first launch of each level records, the next two replay; the three byte strings
    equal each other and the run with the cache off."""
    res = _child(None)
    assert res["stats_env"] is None
    for n_src, r in res["levels"].items():
        s = np.array(r["stats"])
        d = np.diff(s[:, :4], axis=0)
        print(f"counters off, n_src {n_src}: {r['stats']}")
        assert d.tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]], (n_src, r["stats"])
        assert s[1, 4] > s[0, 4] and s[3, 4] == s[1, 4]
        assert r["rule"] == [r["off"]] * 3, n_src


def test_default_rule_counters_on(gpu):
    """The same with PBR_MC_STATS=1: the rule keeps the cache off, nothing records, nothing replays."""
    res = _child("1")
    assert res["stats_env"] == "1"
    for n_src, r in res["levels"].items():
        s = np.array(r["stats"])
        assert (s[:, :2] == 0).all() and (s[:, 4] == 0).all(), (n_src, r["stats"])
        assert r["rule"] == [r["off"]] * 3, n_src
