"""The 32 x 32 x 1-slice tile of the region kernel on the quarter-face shape (k_mc_region.hip, header 2h), forced with
pbrk_mc_set_tile32(1) on a 128^2 source filtered into a 256^2 cube with the roughness-0.03 table (1389 samples), the shape of C4 mip 1
at the smallest output the region kernel accepts (8 x 8 tiles per face).  The tile adds a texel's samples in one chain instead of four
partial sums, so it is held against the direct kernel (the 2e-5 of test_gpu_configs.py), not against the 16 x 16 tile's bytes; among
its own switches (absorb, runs, prologue, launch cut) and between row shards and full dispatches it must give one set of bytes.  A
launch of one slice reports its single cut word in all four entries of pbrk_mc_launch_cut_stats (16 x 16 x 4: four different words),
which is how the cases tell which tile a launch took."""
import ctypes as C

import numpy as np
import pytest

from mc_cases import FULL, OUT, WINDOWS, level as _level
from pbrhip import mc

pytestmark = pytest.mark.gpu

N_SRC, ROUGH = 128, 0.03
ROUGH_LONG = 0.04                                             # 2300 samples: its first 2048 / 2049 are the table-length cases
TOL = 2e-5                                                    # test_c4_every_texel_region_kernel_against_direct_kernel
NO_REGION = {"healed": 0, "slices": 0, "cut4": [0] * 4, "nw": 0, "words_cut": 0}      # what a run of the direct kernel reports


def _bits(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def _run(L, bord, rough, tile32, windows=WINDOWS, n_tab=None, cut=1, direct=False):
    """The windows into one cleared 256^2 cube; returns a dict of the bytes and the counters of the run (cut: the last window's launch)."""
    with mc.switches(L, tile32=tile32, launch_cut=cut, **({"kernels": (0, 0)} if direct else {})):
        mc.reset_counters(L)
        data = mc.filter_windows(L, bord, rough, windows, OUT, n_tab)
        if direct:                                            # the counters exist after the region kernel's first launch
            return {"bytes": data, **NO_REGION, **mc.counters(L, "region", reset=True, missing_ok=True)}
        return {"bytes": data, **mc.counters(L, "cut", "region", reset=True)}


def _one_slice(r):
    """Did the run's last launch take the one-slice tile?  Its four cut entries are one word; four slices own four different ones."""
    return len(set(r["cut4"])) == 1


def _rgb(r):
    return np.frombuffer(r["bytes"], dtype=np.float32).reshape(6, OUT, OUT, 4)


def _worst(a, b):
    """Largest relative difference of the R, G, B of two cubes (floor 1e-3), per texel row: [6, OUT]."""
    err = np.abs(a[..., :3].astype(np.float64) - b[..., :3]) / np.maximum(np.abs(b[..., :3].astype(np.float64)), 1e-3)
    return err.max(axis=(2, 3))


@pytest.fixture(scope="module")
def level(gpu):
    bord = mc.BorderedLevel(gpu, _level(N_SRC))
    yield bord
    bord.free()


@pytest.fixture(scope="module")
def direct_full(gpu, level):
    """The direct kernel over every texel of the cube: computed once, shared, left unchanged."""
    r = _run(gpu, level, ROUGH, 0, FULL, direct=True)
    assert r["slices"] == 0                                   # the region kernel did not run
    a = _rgb(r).copy()
    a.setflags(write=False)
    return a


def test_every_texel_against_the_direct_kernel(gpu, level, direct_full):
    got = _run(gpu, level, ROUGH, 1, FULL)
    assert _one_slice(got) and got["healed"] == 0 and got["slices"] == 6 * (OUT // 32) ** 2 * 16, (got["cut4"], got["healed"], got["slices"])
    a = _rgb(got)
    assert float(np.abs(direct_full[..., :3]).max()) > 0 and np.array_equal(a[..., 3], direct_full[..., 3])
    rows = _worst(a, direct_full)
    # the pole of the tangent frame: face 0 around row floor(0.25 size), face 1 around row floor(0.75 size) (frames twist, most flags)
    p0, p1 = OUT // 4, (3 * OUT) // 4
    pole = max(float(rows[0, p0 - 16:p0 + 16].max()), float(rows[1, p1 - 16:p1 + 16].max()))
    print(f"tile32 against the direct kernel: worst {float(rows.max()):.3e} (pole rows {pole:.3e}), tolerance {TOL:.1e}")
    assert pole < TOL, pole
    assert float(rows.max()) < TOL, float(rows.max())


def test_one_set_of_bytes_over_the_switches(gpu, level):
    L = gpu
    ref = None
    for absorb in (1, 0):
        for runs in (1, 0):
            for prologue in (1, 0):
                for cut in (1, 0):
                    with mc.switches(L, absorb=absorb, runs=runs, prologue=prologue):
                        r = _run(L, level, ROUGH, 1, cut=cut)
                    tag = f"absorb {absorb} runs {runs} prologue {prologue} cut {cut}"
                    assert r["healed"] == 0 and r["slices"] > 0, (tag, r["healed"], r["slices"])
                    assert _one_slice(r), (tag, r["cut4"])
                    if absorb and prologue and cut:
                        assert r["words_cut"] > 0, f"{tag}: nothing cut, the case checks nothing"
                    else:
                        assert r["words_cut"] == 0, tag       # no k_mc_prep result, or the cut switched off: nothing is dropped
                    ref = ref or r
                    assert r["bytes"] == ref["bytes"], tag


@pytest.mark.parametrize("f0,f1", [(0, 1), (1, 2), (3, 4), (0, 2), (4, 6)])
def test_row_shards_equal_the_full_dispatch(gpu, level, f0, f1):
    """Shard boundaries that are no multiples of 32: tiles start at a dispatch's first row, the order of a texel's sum does not."""
    full = _run(gpu, level, ROUGH, 1, [(f0, f1, 0, OUT)])
    shards = _run(gpu, level, ROUGH, 1, [(f0, f1, 0, 37), (f0, f1, 37, 63), (f0, f1, 100, 156)])
    assert _one_slice(full) and _one_slice(shards)
    assert full["words_cut"] > 0 and shards["words_cut"] == full["words_cut"]
    assert full["healed"] == 0 and shards["healed"] == 0
    assert shards["bytes"] == full["bytes"]
    if f1 - f0 == 2:                                          # a face pair against its two single faces
        singles = _run(gpu, level, ROUGH, 1, [(f0, f0 + 1, 0, 100), (f0, f0 + 1, 100, 156), (f0 + 1, f1, 0, 41), (f0 + 1, f1, 41, 215)])
        assert singles["healed"] == 0 and singles["bytes"] == full["bytes"]


@pytest.mark.parametrize("rough,n_tab", [(ROUGH, 1000), (ROUGH_LONG, 2048)])
def test_table_lengths_the_tile_serves(gpu, level, rough, n_tab):
    """1000 samples end inside a mask word; 2048 fill 64 words, the last table one ballot of the run loop covers."""
    assert mc.prefilter_table(gpu, rough)[1] >= n_tab
    got = _run(gpu, level, rough, 1, FULL, n_tab)
    assert _one_slice(got) and got["nw"] == (n_tab + 31) // 32 and got["healed"] == 0 and got["words_cut"] > 0, (got["cut4"], got["nw"], got["healed"])
    off = _run(gpu, level, rough, 1, FULL, n_tab, cut=0)
    assert off["words_cut"] == 0 and off["healed"] == 0 and off["bytes"] == got["bytes"]
    want = _rgb(_run(gpu, level, rough, 0, FULL, n_tab, direct=True))
    worst = float(_worst(_rgb(got), want).max())
    print(f"n_tab {n_tab}: tile32 against the direct kernel: worst {worst:.3e}, tolerance {TOL:.1e}")
    assert worst < TOL, worst


def test_longer_tables_and_whole_faces_keep_the_16_tile(gpu, level):
    """2049 samples are 65 mask words: the level falls back to 16 x 16 x 4 and gives the bytes of pbrk_mc_set_tile32(0); so does the
    whole-face shape (n_src = 64), whatever the table."""
    assert mc.prefilter_table(gpu, ROUGH_LONG)[1] >= 2049
    forced = _run(gpu, level, ROUGH_LONG, 1, n_tab=2049)
    never = _run(gpu, level, ROUGH_LONG, 0, n_tab=2049)
    assert not _one_slice(forced) and forced["nw"] == 65 and forced["healed"] == 0 and never["healed"] == 0
    assert forced["bytes"] == never["bytes"]
    whole = mc.BorderedLevel(gpu, _level(64))
    try:
        forced = _run(gpu, whole, 0.15, 1)
        never = _run(gpu, whole, 0.15, 0)
    finally:
        whole.free()
    assert not _one_slice(forced) and forced["healed"] == 0 and never["healed"] == 0 and forced["slices"] > 0
    assert forced["bytes"] == never["bytes"]


def _host_cut(L, rough, lvl):
    """pbrk_mc_launch_cut_slices with one slice, fed with the level's extrema: every texel of the bordered level is a texel of the
    level or a mean of such, so they are the extrema k_mc_prep finds."""
    tab = np.zeros((8192, 4), dtype=np.float32)
    alpha = C.c_float()
    n = L.pbrk_host_prefilter_table(8192, rough, tab.ctypes.data_as(C.c_void_p), C.byref(alpha))
    w = np.ascontiguousarray(tab[:n, 3])
    cut = (C.c_int * 4)()
    k = L.pbrk_mc_launch_cut_slices(w.ctypes.data_as(C.POINTER(C.c_float)), n, 1, _bits(lvl[..., :3].min()), _bits(lvl[..., :3].max()), cut)
    return k, cut[0]


def test_reported_cut_is_the_host_twin(gpu, level):
    L = gpu
    k, c = _host_cut(L, ROUGH, _level(N_SRC))
    clean = _run(L, level, ROUGH, 1)
    assert k > 0 and clean["cut4"] == [c] * 4 and clean["words_cut"] == k, (clean["cut4"], clean["words_cut"], c, k)
    # a 1e5:1 bright 4 x 4 patch: the level's maximum is its peak, the proof holds for fewer words -- and still exactly
    lvl = _level(N_SRC)
    lvl[2, 10:14, 10:14, :3] *= 1e5
    kb, cb = _host_cut(L, ROUGH, lvl)
    bord = mc.BorderedLevel(L, lvl)
    try:
        bright = _run(L, bord, ROUGH, 1)
        off = _run(L, bord, ROUGH, 1, cut=0)
    finally:
        bord.free()
    assert bright["cut4"] == [cb] * 4 and bright["words_cut"] == kb
    assert 0 < bright["words_cut"] < clean["words_cut"] and cb > c
    assert bright["bytes"] == off["bytes"] and bright["healed"] == 0 and off["healed"] == 0


@pytest.mark.parametrize("where", ["inside", "apron"])
def test_negative_or_minus_zero_texel_switches_the_cut_off(gpu, where):
    """By bit pattern both order above +inf: the level's maximum is no finite float and no word is cut; the bytes stay those without."""
    L = gpu
    y = 20 if where == "inside" else 64
    for ch, bad in ((1, -1e-6), (2, -0.0)):
        lvl = _level(N_SRC)
        lvl[4, y, 20, ch] = bad
        bord = mc.BorderedLevel(L, lvl)
        try:
            on = _run(L, bord, ROUGH, 1)
            off = _run(L, bord, ROUGH, 1, cut=0)
        finally:
            bord.free()
        assert _one_slice(on) and on["words_cut"] == 0 and off["words_cut"] == 0, (where, bad, on["cut4"])
        assert on["bytes"] == off["bytes"] and on["healed"] == 0 and off["healed"] == 0


def test_default_rule_keeps_the_16_tile_on_a_256_cube(gpu, level):
    """The rule (-1) asks for an output of at least the measured size: a 256^2 level keeps 16 x 16 x 4 and the bytes it had."""
    default = _run(gpu, level, ROUGH, -1)
    never = _run(gpu, level, ROUGH, 0)
    assert not _one_slice(default) and default["words_cut"] > 0 and default["healed"] == 0 and never["healed"] == 0
    assert default["bytes"] == never["bytes"]
    assert _run(gpu, level, ROUGH, 1)["bytes"] != default["bytes"]      # the forced tile is another order of the same sum
