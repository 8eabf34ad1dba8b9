"""half_n folded into the permuted frame rows of the region kernel's run loop (k_mc_region.hip, header 2j; pbrk_mc_set_fold) against
the loop that keeps the multiply: on levels whose edge is a power of two the folded instantiation runs and gives the same bytes;
on every other level the switch changes nothing, the launch reports no fold.  pbrk_mc_last_fold() tells which instantiation the last
launch took.

256^2 outputs, the smallest the region kernel accepts: proved runs are short and mixed with tested samples there, so both folded
bodies (proved and tested) and the count-only body of absorbed words run.  Tables: the whole table of the roughness, 1000 samples
(the last mask word ragged) and 100 (at most one word per slice)."""
import numpy as np
import pytest

from mc_cases import FULL, OUT, WINDOWS, level
from pbrhip import mc

pytestmark = pytest.mark.gpu

# (n_src, roughness, tile32): 66^2 whole face; 34^2; quarter faces with the 16 x 16 x 4 and the 32 x 32 x 1 tile; two levels whose
# half_n is no power of two (66^2 and 34^2 partly filled)
SHAPES = [(64, 0.15, 0), (32, 0.4, 0), (128, 0.03, 0), (128, 0.03, 1), (48, 0.15, 0), (24, 0.4, 0)]
TABLES = [None, 1000, 100]
ROW_WINDOWS = [WINDOWS[0], WINDOWS[2]]


def _pow2(n):
    return n & (n - 1) == 0


def _run(L, bord, rough, n_tab, tile32, windows=FULL, **sw):
    """One dispatch set into a cleared cube under the named switches: (bytes, counters, pbrk_mc_last_fold())."""
    with mc.switches(L, tile32=tile32, **sw):
        mc.reset_counters(L)
        data = mc.filter_windows(L, bord, rough, windows, OUT, n_tab)
        fold = L.pbrk_mc_last_fold()
        return data, mc.counters(L, "window", "flag", "region", reset=True), fold


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"n{s[0]}t{s[2]}")
def shape(request, gpu):
    n_src, rough, tile32 = request.param
    bord = mc.BorderedLevel(gpu, level(n_src))
    ones = mc.BorderedLevel(gpu, np.ones((6, n_src, n_src, 4), np.float32))
    yield n_src, rough, tile32, bord, ones
    bord.free()
    ones.free()


@pytest.mark.parametrize("n_tab", TABLES, ids=lambda n: f"tab{n or 'full'}")
def test_fold_keeps_the_bytes(gpu, shape, n_tab):
    L = gpu
    n_src, rough, tile32, bord, ones = shape
    n_full = mc.prefilter_table(L, rough)[1]
    assert n_full > 1000, n_full
    out = {}
    for fold in (0, 1):
        for absorb in (0, 1):
            data, c, took = _run(L, bord, rough, n_tab, tile32, fold=fold, absorb=absorb)
            print(f"n_src {n_src} tile32 {tile32} n_tab {n_tab or n_full} fold {fold} absorb {absorb}: folded launch {took}, "
                  f"proved {c['proved']} of {c['flag_samples']}, healed {c['healed']} of {c['slices']}")
            out[fold, absorb] = (mc.digest(np.frombuffer(data, np.uint8)), c, took)
    # 1. one SHA-256 of the whole cube, fold on and off, absorb on and off (off a power of two: the switch changes nothing at all)
    assert len({d for d, _, _ in out.values()}) == 1, {k: d for k, (d, _, _) in out.items()}
    for (fold, absorb), (_, c, took) in out.items():
        # 2. the folded instantiation ran exactly where the level allows it and the switch asks for it
        assert took == (1 if fold and _pow2(n_src) else 0), (fold, absorb, took)
        # 3. the completeness check never recomputed a wave-slice, and proved runs were taken
        assert c["healed"] == 0 and c["slices"] > 0, (fold, absorb, c)
        assert c["proved"] > 0, (fold, absorb, c)
    # 4. ragged row windows equal those rows of the full dispatch, fold on; a row shard takes the instantiation of its level
    full, c, took = _run(L, bord, rough, n_tab, tile32, fold=1)
    assert mc.digest(np.frombuffer(full, np.uint8)) == out[1, 1][0]
    full = np.frombuffer(full, np.float32).reshape(6, OUT, OUT, 4)
    for window in ROW_WINDOWS:
        win, c, took = _run(L, bord, rough, n_tab, tile32, [window], fold=1)
        win = np.frombuffer(win, np.float32).reshape(6, OUT, OUT, 4)
        f0, f1, y0, rows = window
        assert took == (1 if _pow2(n_src) else 0), (window, took)
        assert c["healed"] == 0 and c["slices"] > 0, (window, c)
        assert win[f0:f1, y0:y0 + rows].tobytes() == full[f0:f1, y0:y0 + rows].tobytes(), window
    # 5. a level of all ones: every (texel, sample) pair exactly once, so a pair taken twice or missed would change the sum
    flat = {}
    for fold in (0, 1):
        data, c, took = _run(L, ones, rough, n_tab, tile32, fold=fold)
        assert c["healed"] == 0 and c["slices"] > 0, (fold, c)
        assert took == (1 if fold and _pow2(n_src) else 0), (fold, took)
        flat[fold] = data
    assert flat[0] == flat[1]


def test_no_fold_without_the_lean_run_loop(gpu):
    """The folded instantiations exist for the lean run loop alone: runs or prologue off, the launch reports none and the bytes stay."""
    L = gpu
    bord = mc.BorderedLevel(L, level(64))
    try:
        want, c, took = _run(L, bord, 0.15, 1000, 0)
        assert took == 1 and c["healed"] == 0
        for sw in ({"runs": 0}, {"prologue": 0}):
            data, c, took = _run(L, bord, 0.15, 1000, 0, **sw)
            assert took == 0 and c["healed"] == 0 and c["slices"] > 0, (sw, took, c)
            assert data == want, sw
    finally:
        bord.free()
