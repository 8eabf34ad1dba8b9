"""The launch-level cut of the region kernel (k_mc_region.hip, header 2g): each slice's head word runs first over every region, and the
tail words k_mc_cut proves to be no-ops for every lane of the launch are not binned at all.  Dropping them is exact, so the output
bytes with the cut (pbrk_mc_set_launch_cut(1), the default) must be those without it -- on both 66^2 shapes, with absorbed-word
skipping, the round-5 loop and the lean prologue on and off (the cut exists only where k_mc_prep ran: absorb and prologue on), with
nothing healed, and with no fewer absorbed wave-samples in the counters.  Row windows of 256^2 levels through pbrk_mc_filter, as in
test_gpu_mc_prologue.py."""
import pytest

from mc_cases import OUT, WINDOWS, level
from pbrhip import mc

pytestmark = pytest.mark.gpu

# (n_src, roughness): quarter faces with the 1389-sample table, whole faces with the 8192-sample table
SHAPES = [(128, 0.03), (64, 0.15)]


def _run(L, bord, rough, cut, n_tab=None, windows=WINDOWS):
    """The windows into one cleared 256^2 cube with the launch cut on or off; returns a dict of the bytes and the counters (cut: the
    last window's launch)."""
    with mc.switches(L, launch_cut=cut):
        mc.reset_counters(L)
        data = mc.filter_windows(L, bord, rough, windows, OUT, n_tab)
        return {"bytes": data, **mc.counters(L, "skip", "cut", "region", reset=True)}


def _on_off(L, bord, rough, absorb=1, runs=1, prologue=1, n_tab=None, windows=WINDOWS):
    """Cut on against cut off under one setting of the other switches.  Returns (on, off)."""
    with mc.switches(L, absorb=absorb, runs=runs, prologue=prologue):
        on = _run(L, bord, rough, 1, n_tab, windows)
        off = _run(L, bord, rough, 0, n_tab, windows)
    tag = f"n_src {bord.n_src} absorb {absorb} runs {runs} prologue {prologue}"
    assert on["bytes"] == off["bytes"], f"{tag}: the launch cut changed the output bytes"
    assert on["healed"] == 0 and off["healed"] == 0 and on["slices"] > 0 and off["slices"] == on["slices"], (tag, on["healed"], off["healed"])
    assert off["words_cut"] == 0, tag
    if absorb and prologue:
        assert on["words_cut"] > 0, f"{tag}: nothing cut, the case checks nothing"
        assert on["abs_samples"] >= off["abs_samples"], (tag, on["abs_samples"], off["abs_samples"])
    else:
        assert on["words_cut"] == 0, tag                       # no k_mc_prep result: nothing is dropped
    return on, off


@pytest.mark.parametrize("n_src,rough", SHAPES)
def test_cut_on_equals_cut_off(gpu, n_src, rough):
    bord = mc.BorderedLevel(gpu, level(n_src))
    try:
        ref = None
        for absorb in (1, 0):
            for runs in (1, 0):
                for prologue in (1, 0):
                    on, _ = _on_off(gpu, bord, rough, absorb, runs, prologue)
                    ref = ref or on
                    assert on["bytes"] == ref["bytes"], (absorb, runs, prologue)      # one set of bytes whatever the switches
    finally:
        bord.free()


@pytest.mark.parametrize("n_src,rough", SHAPES)
def test_table_length_no_multiple_of_32(gpu, n_src, rough):
    """A table that ends inside a mask word: the last word of one slice is short, in the kernel's count of a slice's samples too."""
    _, n_full, _ = mc.prefilter_table(gpu, rough)
    n_tab = n_full - 13
    if n_tab % 32 == 0:
        n_tab -= 1
    assert n_tab > 160 and n_tab % 32 != 0
    bord = mc.BorderedLevel(gpu, level(n_src))
    try:
        for absorb, runs in ((1, 1), (1, 0), (0, 1)):
            _on_off(gpu, bord, rough, absorb, runs, 1, n_tab)
    finally:
        bord.free()


@pytest.mark.parametrize("n_src,rough", SHAPES)
def test_bright_patch_cuts_later(gpu, n_src, rough):
    """A 1e5:1 bright 4 x 4 patch: the level's maximum is its peak, so the proof holds for fewer words -- and still exactly."""
    bord = mc.BorderedLevel(gpu, level(n_src))
    try:
        clean, _ = _on_off(gpu, bord, rough)
    finally:
        bord.free()
    lvl = level(n_src)
    lvl[2, 10:14, 10:14, :3] *= 1e5
    bord = mc.BorderedLevel(gpu, lvl)
    try:
        bright, _ = _on_off(gpu, bord, rough)
    finally:
        bord.free()
    assert 0 < bright["words_cut"] < clean["words_cut"], (bright["words_cut"], clean["words_cut"])
    assert all(b > c for b, c in zip(bright["cut4"], clean["cut4"])), (bright["cut4"], clean["cut4"])


@pytest.mark.parametrize("n_src,rough", SHAPES)
@pytest.mark.parametrize("where", ["inside", "apron"])
def test_negative_or_minus_zero_texel_switches_the_cut_off(gpu, n_src, rough, where):
    """One small negative component and one -0.0 -- inside a face, and in the last texel row a region stages (the apron): by bit
    pattern both order above +inf, the level's maximum is no finite float and no word is cut.  The bytes stay those without the cut."""
    L = gpu
    y = 20 if where == "inside" else (64 if n_src > 65 else n_src - 1)
    for ch, bad in ((1, -1e-6), (2, -0.0)):
        lvl = level(n_src)
        lvl[4, y, 20, ch] = bad
        bord = mc.BorderedLevel(L, lvl)
        try:
            on = _run(L, bord, rough, 1)
            off = _run(L, bord, rough, 0)
        finally:
            bord.free()
        assert on["words_cut"] == 0 and off["words_cut"] == 0, (where, bad, on["cut4"])
        assert on["bytes"] == off["bytes"] and on["healed"] == 0 and off["healed"] == 0


@pytest.mark.parametrize("n_src,rough", SHAPES)
def test_row_shards_equal_the_full_dispatch(gpu, n_src, rough):
    """The order of a texel's sum (phase, region as visited, sample index) and the cut depend on the launch's level and table only: ragged
    row shards of two faces give the bytes of one dispatch over the same rows."""
    bord = mc.BorderedLevel(gpu, level(n_src))
    try:
        full = _run(gpu, bord, rough, 1, windows=[(0, 2, 40, 120)])
        shards = _run(gpu, bord, rough, 1, windows=[(0, 1, 40, 37), (0, 1, 77, 83), (1, 2, 40, 16), (1, 2, 56, 51), (1, 2, 107, 53)])
    finally:
        bord.free()
    assert full["words_cut"] > 0 and shards["words_cut"] > 0
    assert full["healed"] == 0 and shards["healed"] == 0
    assert shards["bytes"] == full["bytes"]
