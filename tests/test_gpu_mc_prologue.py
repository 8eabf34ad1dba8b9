"""The lean prologue of the region kernel (k_mc_region.hip, header 2f: the maxima of the absorbed-word test from a preparation
kernel once per launch, binning without run-time divisions, row-wise staging) against the prologue it replaces
(pbrk_mc_set_prologue(0)): the output bytes must be the same on every region shape, with absorbed-word skipping and the round-5
loop on and off, and the completeness self-check must never recompute a wave-slice.  Row windows of 256^2 levels, the smallest
the region kernel accepts, driven through pbrk_mc_filter."""
import ctypes as C

import numpy as np
import pytest

from mc_cases import OUT, WINDOWS, level
from pbrhip import mc

pytestmark = pytest.mark.gpu

# (n_src, roughness): 18^2, 34^2, 66^2 whole face, 66^2 with rows not contiguous in LDS (nb < RS), quarter faces, G == 2 with a short
# last region of 36 cells
SHAPES = [(16, 0.6), (32, 0.4), (64, 0.15), (48, 0.15), (128, 0.03), (100, 0.03)]
BIG = [(64, 0.15), (48, 0.15), (128, 0.03), (100, 0.03)]            # the 66^2 shapes: absorbed words, round-5 loop


def _run(L, bord, rough, n_tab=None):
    """All windows into one cleared 256^2 cube; returns (bytes, healed wave-slices, wave-slices, absorbed wave-words)."""
    mc.reset_counters(L)
    data = mc.filter_windows(L, bord, rough, WINDOWS, OUT, n_tab)
    c = mc.counters(L, "skip", "region", reset=True)
    return data, c["healed"], c["slices"], c["abs_words"]


def _both(L, bord, rough, absorb=1, runs=1, n_tab=None):
    """The same dispatches with the lean prologue and with the one before it: equal bytes, nothing healed.  Returns the lean run."""
    with mc.switches(L, absorb=absorb, runs=runs):
        new = _run(L, bord, rough, n_tab)
        with mc.switches(L, prologue=0):
            old = _run(L, bord, rough, n_tab)
    assert new[0] == old[0], f"n_src {bord.n_src} absorb {absorb} runs {runs}: the lean prologue changed the output bytes"
    assert new[1] == 0 and old[1] == 0 and new[2] > 0 and old[2] > 0, (new[1:], old[1:])
    return new


@pytest.mark.parametrize("n_src,rough", SHAPES)
def test_lean_prologue_equals_parent(gpu, n_src, rough):
    bord = mc.BorderedLevel(gpu, level(n_src))
    try:
        for absorb in (1, 0):
            for runs in ((1, 0) if (n_src, rough) in BIG else (1,)):
                _both(gpu, bord, rough, absorb, runs)
    finally:
        bord.free()


@pytest.mark.parametrize("n_src,rough", BIG)
def test_bright_patch(gpu, n_src, rough):
    """A 1e5:1 bright 4 x 4 patch in one face: the region maximum is its peak, lanes near it absorb far more than the others."""
    lvl = level(n_src)
    lvl[2, 10:14, 10:14, :3] *= 1e5
    bord = mc.BorderedLevel(gpu, lvl)
    try:
        for absorb in (1, 0):
            _both(gpu, bord, rough, absorb)
    finally:
        bord.free()


@pytest.mark.parametrize("n_src,rough", BIG)
@pytest.mark.parametrize("where", ["inside", "apron"])
def test_negative_and_minus_zero_switch_region_off(gpu, n_src, rough, where):
    """One small negative component and one -0.0: by bit pattern both order above +inf, so their region must stop absorbing --
    inside a region, and in the last texel row a region stages (the first row of the region below it, or the face's border)."""
    L = gpu
    bord = mc.BorderedLevel(L, level(n_src))
    try:
        clean = _both(L, bord, rough)
    finally:
        bord.free()
    lvl = level(n_src)
    y = 20 if where == "inside" else (64 if n_src > 65 else n_src - 1)   # bordered row y + 1: row 65 of region gy = 0, or the last row of the face
    lvl[4, y, 20, 1] = -1e-6
    lvl[4, y, 30, 2] = -0.0
    bord = mc.BorderedLevel(L, lvl)
    try:
        patched = _both(L, bord, rough)
    finally:
        bord.free()
    assert clean[3] > 0, "nothing absorbed on the clean level: the case checks nothing"
    assert patched[3] < clean[3], (patched[3], clean[3])


@pytest.mark.parametrize("n_src,rough", BIG)
def test_table_length_no_multiple_of_32(gpu, n_src, rough):
    """A table that ends inside a mask word: the word's maximum must come from the samples it holds alone."""
    _, n_full, _ = mc.prefilter_table(gpu, rough)
    n_tab = n_full - 13
    if n_tab % 32 == 0:
        n_tab -= 1
    assert n_tab > 32 and n_tab % 32 != 0
    bord = mc.BorderedLevel(gpu, level(n_src))
    try:
        for absorb in (1, 0):
            _both(gpu, bord, rough, absorb, 1, n_tab)
    finally:
        bord.free()


def test_dispatches_in_flight_on_several_streams(gpu):
    """Row windows of two levels of different region shapes (mip 1: quarter faces of a 128^2 source, mip 2: whole 64^2 faces), 36
    dispatches dealt over four tile streams -- more than the scratch ring has slots -- against the same dispatches in order on one."""
    import pbrhip
    L = gpu
    S = 1024
    tex = mc.env_texture(np.random.default_rng(11).random((6, 2048, 2048, 4), dtype=np.float32) + 0.1)
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), 8, 64, S)
    spec = maps.tex_specular_env_map
    pipes = L.PBR_MakeIBLPipelines(); arena = L.GPU_MakeDescriptorArena(); g = L.GPU_MakeGraph()
    units = []
    for f in range(6):
        for k in range(3):
            for m in (1, 2):
                y0 = 16 * (f + 2 * k)
                units.append(pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, m, f, f + 1, y0, y0 + 16 + k, 0.0))
    arr = (pbrhip.PBR_WorkUnit * len(units))(*units)

    def run(streams):
        L.GPUX_SetTileStreams(streams)
        for m in (1, 2):
            L.GPU_OpClearColorF(g, spec, m, 0.0, 0.0, 0.0, 0.0)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        mc.reset_counters(L)
        L.PBR_RecordUnits(pipes, g, arena, tex, C.byref(maps), arr, len(units))
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g); L.GPU_ResetDescriptorArena(arena)
        st = mc.counters(L, "region", reset=True)
        assert st["healed"] == 0 and st["slices"] > 0, (st["healed"], st["slices"])
        return [mc.digest(pbrhip.read_mip(spec, m)) for m in (1, 2)]

    try:
        serial = run(0)
        assert run(4) == serial
        with mc.switches(L, prologue=0):
            assert run(4) == serial
    finally:
        L.GPUX_SetTileStreams(-1)
        L.GPU_DestroyGraph(g); L.GPU_DestroyDescriptorArena(arena); L.PBR_DestroyIBLPipelines(pipes)
        L.PBR_DestroyIBLMaps(C.byref(maps))
        L.GPU_DestroyTexture(tex)
