"""The round-5 loop of the region kernel (k_mc_region.hip, RUNS: non-empty words only, runs of proved samples, per-lane counts,
a barrier per visited region only) against the loop it replaces (pbrk_mc_set_runs(0)): the outputs must be the same bytes, with
absorbed-word skipping on and off, and the completeness self-check must never recompute a wave-slice."""
import ctypes as C

import pytest

import pbrhip
from pbrhip import mc

pytestmark = pytest.mark.gpu

C4_S, C4_MIN = 4096, 128


def _healed(L):
    c = mc.counters(L, "region", reset=True)
    return c["healed"], c["slices"]


def _chain(L, env, runs, absorb, S=C4_S, min_size=C4_MIN, mips=(1, 2, 3, 4)):
    tex = mc.env_texture(env)
    spec = pbrhip.make_texture(pbrhip.Format_RGBA32F, S, S, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps | pbrhip.TextureFlag_StorageImage)
    try:
        with mc.switches(L, runs=runs, absorb=absorb):
            mc.reset_counters(L)
            L.PBR_GenPrefilteredEnvMap(tex, spec, min_size)
            L.GPU_WaitUntilIdle()
            healed = _healed(L)
            return {m: mc.digest(pbrhip.read_mip(spec, m)) for m in mips}, healed
    finally:
        L.GPU_DestroyTexture(spec)
        L.GPU_DestroyTexture(tex)


def _same(L, env, **kw):
    for absorb in (1, 0):
        new, h_new = _chain(L, env, 1, absorb, **kw)
        old, h_old = _chain(L, env, 0, absorb, **kw)
        assert new == old, f"absorb {absorb}: the round-5 loop changed the output bytes"
        assert h_new[0] == 0 and h_old[0] == 0 and h_new[1] > 0, (h_new, h_old)


def test_c4_runs_equal_old_loop(gpu, c4_env):
    """C4 at full size: mips 1 (quarter-face regions) and 2 (whole faces) take the new loop; 3 and 4 never do."""
    _same(gpu, c4_env)


def test_bright_sun_and_tolerance_cut_tables(gpu, c4_env):
    """A 1e5:1 sun patch (absorbs differently per lane), then tables cut by GPUX_SetPrefilterTolerance."""
    L = gpu
    env = c4_env.copy()
    env[4, 1000:1008, 1000:1008, :3] *= 1e5
    _same(L, env)
    try:
        L.GPUX_SetPrefilterTolerance(1e-7)
        _same(L, c4_env)
    finally:
        L.GPUX_SetPrefilterTolerance(0.0)


def test_ragged_row_shards_with_runs(gpu, c4_env):
    """Rows that are no multiple of the 16-row tile, three shards per face: the same bytes as the old loop's whole-level dispatch."""
    L = gpu
    tex = mc.env_texture(c4_env)
    pipes = L.PBR_MakeIBLPipelines(); arena = L.GPU_MakeDescriptorArena(); g = L.GPU_MakeGraph()
    try:
        for S, mips in ((512, (1,)), (C4_S, (1, 2))):
            maps = pbrhip.PBR_IBLMaps()
            L.PBR_MakeIBLMaps(C.byref(maps), 8, 64, S)
            spec = maps.tex_specular_env_map
            with mc.switches(L, runs=0):
                L.PBR_GenPrefilteredEnvMap(tex, spec, 256)
                L.GPU_WaitUntilIdle()
                full = {m: mc.digest(pbrhip.read_mip(spec, m)) for m in mips}
            for m in mips:
                L.GPU_OpClearColorF(g, spec, m, 0.0, 0.0, 0.0, 0.0)
            L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
            units = []
            for m in mips:
                size = S >> m
                for f in range(6):
                    cuts = (0, 5 + f, 131 - 2 * f, size)
                    units += [pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, m, f, f + 1, cuts[k], cuts[k + 1], 0.0) for k in range(3)]
            arr = (pbrhip.PBR_WorkUnit * len(units))(*units)
            mc.reset_counters(L)
            L.PBR_RecordUnits(pipes, g, arena, tex, C.byref(maps), arr, len(units))
            L.GPU_GraphSubmit(g); L.GPU_GraphWait(g); L.GPU_ResetDescriptorArena(arena)
            assert _healed(L)[0] == 0
            for m in mips:
                assert mc.digest(pbrhip.read_mip(spec, m)) == full[m], (S, m)
            L.PBR_DestroyIBLMaps(C.byref(maps))
    finally:
        L.GPU_DestroyGraph(g); L.GPU_DestroyDescriptorArena(arena); L.PBR_DestroyIBLPipelines(pipes)
        L.GPU_DestroyTexture(tex)


def _faces(L, tex, S, mips, faces, runs):
    """Faces [f0, f1) of the given mips dispatched alone; returns {mip: digest of those faces} and the healed counters."""
    units = [pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, m, faces[0], faces[1], 0, S >> m, 0.0) for m in mips]
    with mc.switches(L, runs=runs), mc.dispatch_prefilter_units(L, tex, S, units) as maps:
        healed = _healed(L)
        return {m: mc.digest(pbrhip.read_mip(maps.tex_specular_env_map, m)[faces[0]:faces[1]]) for m in mips}, healed


def test_pole_faces_alone(gpu, c4_env):
    """Faces +-X dispatched on their own: the tiles around the tangent frame's pole flag the most regions (a sample in several
    regions, sparse words in the neighbours), and the dispatch starts with them."""
    L = gpu
    tex = mc.env_texture(c4_env)
    try:
        for absorb in (1, 0):
            with mc.switches(L, absorb=absorb):
                new, h_new = _faces(L, tex, C4_S, (1, 2), (0, 2), 1)
                old, h_old = _faces(L, tex, C4_S, (1, 2), (0, 2), 0)
            assert new == old, absorb
            assert h_new[0] == 0 and h_old[0] == 0 and h_new[1] > 0, (h_new, h_old)
    finally:
        L.GPU_DestroyTexture(tex)
