"""Test-free runs of proved samples on the whole-face shapes of the region kernel (k_mc_region.hip, header 2i: under the round-5
loop, the samples binning proves to tap one face from every texel of the tile run without the in-face test, the exec mask and
the per-lane count) against the loops they replace: pbrk_mc_set_runs(0) is the byte yardstick, with both prologues.

256^2 outputs, the smallest the region kernel accepts: a 16 x 16 tile spans 4, 2 or 1 source texels there, its frames spread four
times as far as on C4 mip 2, so proved runs are short and mixed with tested samples -- where a run boundary or a credit can go
wrong.  Tables: the whole table of the roughness (up to 8192 samples), 1000 samples (the last mask word ragged) and 100 (at most
one word per slice)."""
import numpy as np
import pytest

from mc_cases import FULL, OUT, level
from pbrhip import mc

pytestmark = pytest.mark.gpu

# (n_src, roughness, region edge RS): 66^2 full; 66^2 partly filled, half_n no power of two; 34^2; 34^2 partly filled; 18^2
SHAPES = [(64, 0.15, 66), (48, 0.15, 66), (32, 0.4, 34), (24, 0.4, 34), (16, 0.6, 18)]
TABLES = [None, 1000, 100]
# the region shapes whose round-5 loop runs the proved samples test-free (k_mc_region.hip, header 2i: MC_CERT_G1 and the 34^2 shape)
PROVED_RUNS = {66, 34}
WINDOW = (0, 2, 48, 32)


def _run(L, bord, rough, n_tab, windows=FULL):
    """One dispatch set into a cleared cube: (bytes, counters)."""
    mc.reset_counters(L)
    data = mc.filter_windows(L, bord, rough, windows, OUT, n_tab)
    return data, mc.counters(L, "window", "flag", "region", reset=True)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"n{s[0]}")
def shape(request, gpu):
    n_src, rough, rs = request.param
    bord = mc.BorderedLevel(gpu, level(n_src))
    ones = mc.BorderedLevel(gpu, np.ones((6, n_src, n_src, 4), np.float32))
    yield n_src, rough, rs, bord, ones
    bord.free()
    ones.free()


@pytest.mark.parametrize("n_tab", TABLES, ids=lambda n: f"tab{n or 'full'}")
def test_proved_runs_keep_the_bytes(gpu, shape, n_tab):
    L = gpu
    n_src, rough, rs, bord, ones = shape
    n_full = mc.prefilter_table(L, rough)[1]
    assert n_full > 1000, n_full
    runs_out = {}
    for runs in (0, 1):
        for prologue in (0, 1):
            with mc.switches(L, runs=runs, prologue=prologue):
                data, c = _run(L, bord, rough, n_tab)
            print(f"n_src {n_src} n_tab {n_tab or n_full} runs {runs} prologue {prologue}: proved {c['proved']} of {c['flag_samples']}, "
                  f"healed {c['healed']} of {c['slices']}")
            runs_out[runs, prologue] = (mc.digest(np.frombuffer(data, np.uint8)), c)
    # 1. one SHA-256 of the whole cube for the four builds of the loop
    assert len({d for d, _ in runs_out.values()}) == 1, {k: d for k, (d, _) in runs_out.items()}
    for (runs, prologue), (_, c) in runs_out.items():
        # 4. the completeness check never recomputed a wave-slice
        assert c["healed"] == 0 and c["slices"] > 0, (runs, prologue, c)
        assert c["flag_samples"] > 0, (runs, prologue, c)
        if runs and rs in PROVED_RUNS:
            # 5. the proved path is taken, and not for every sample
            assert 0 < c["proved"] < c["flag_samples"], (runs, prologue, c)
        else:
            # 6. the loop before it (and a shape without proved runs) reports none, as before
            assert c["proved"] == 0, (runs, prologue, c)
    # 2. a row window equals those rows of the full dispatch
    full = np.frombuffer(_run(L, bord, rough, n_tab)[0], np.float32).reshape(6, OUT, OUT, 4)
    win, c = _run(L, bord, rough, n_tab, [WINDOW])
    win = np.frombuffer(win, np.float32).reshape(6, OUT, OUT, 4)
    f0, f1, y0, rows = WINDOW
    assert c["healed"] == 0 and c["slices"] > 0, c
    assert win[f0:f1, y0:y0 + rows].tobytes() == full[f0:f1, y0:y0 + rows].tobytes()
    # 3. a level of all ones: every (texel, sample) pair exactly once, so a double or a missed credit would change the sum
    flat = {}
    for runs in (0, 1):
        with mc.switches(L, runs=runs):
            data, c = _run(L, ones, rough, n_tab)
        assert c["healed"] == 0 and c["slices"] > 0, (runs, c)
        flat[runs] = data
    assert flat[0] == flat[1]
