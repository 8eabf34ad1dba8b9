"""Absorbed words of the region kernel (k_mc_region.hip, 2c): a mask word whose samples provably cannot change any lane's fp32 sums
is skipped.  The outputs must not move by a single bit: every case here runs with skipping on and off (pbrk_mc_set_absorb) and
compares the raw bytes, and the kernel's completeness self-check must never have to recompute a wave-slice."""
import ctypes as C

import numpy as np
import pytest

import pbrhip
from pbrhip import mc

pytestmark = pytest.mark.gpu

C4_W, C4_S, C4_MIN = 2048, 4096, 128          # bench C4: 2048^2 environment -> 4096^2 prefiltered cube, Monte-Carlo mips 1..5


def _healed(L):
    c = mc.counters(L, "region")
    return c["healed"], c["slices"]


def _skips(L):
    c = mc.counters(L, "skip", "flag")
    return c["abs_words"], c["abs_samples"], c["count_only"], 4 * c["flags"]      # words, samples, count-only samples, wave-samples visited


def _prefilter(L, tex, S, min_size, absorb, mips):
    """Whole chain with skipping on / off; returns {mip: sha256 of the raw bytes} and the counters of the run."""
    spec = pbrhip.make_texture(pbrhip.Format_RGBA32F, S, S, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps | pbrhip.TextureFlag_StorageImage)
    try:
        with mc.switches(L, absorb=absorb):
            mc.reset_counters(L)
            L.PBR_GenPrefilteredEnvMap(tex, spec, min_size)
            L.GPU_WaitUntilIdle()
            counters = (_healed(L), _skips(L))
            out = {}
            for m in mips:
                a = pbrhip.read_mip(spec, m)
                out[m] = (mc.digest(a), float(np.abs(a[..., :3]).max()) if np.isfinite(a[..., :3]).all() else None)
    finally:
        L.GPU_DestroyTexture(spec)
    return out, counters


def _per_mip_skips(L, tex, S, mip):
    """One level dispatched on its own (skipping on): the counters of that level alone."""
    with mc.dispatch_prefilter_units(L, tex, S, [pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, mip, 0, 6, 0, S >> mip, 0.0)]):
        return _healed(L), _skips(L)


def _on_off(L, env, S=C4_S, min_size=C4_MIN, mips=(1, 2, 3, 4, 5)):
    tex = mc.env_texture(env)
    try:
        on, c_on = _prefilter(L, tex, S, min_size, 1, mips)
        off, c_off = _prefilter(L, tex, S, min_size, 0, mips)
    finally:
        L.GPU_DestroyTexture(tex)
    for m in mips:
        assert on[m][0] == off[m][0], f"mip {m}: skipping changed the output bytes"
    assert c_on[0][0] == 0 and c_off[0][0] == 0 and c_on[0][1] > 0, (c_on, c_off)      # no healed wave-slice, the kernel ran
    assert c_off[1][:3] == (0, 0, 0), c_off
    return on, c_on[1]


def test_c4_skip_on_equals_off_and_skips_on_mips_1_2(gpu, c4_env):
    """C4 at full size (mips 1-5 of the 4096^2 cube): bit-identical with and without skipping; mips 1 and 2 skip words, and the
    measured skip fraction per level is printed next to the counters."""
    L = gpu
    on, sk = _on_off(L, c4_env)
    assert all(on[m][1] and on[m][1] > 0 for m in (1, 2, 3, 4)), on
    assert sk[0] > 0 and 0 < sk[1] <= sk[3] and sk[2] <= sk[1], sk
    tex = mc.env_texture(c4_env)
    try:
        for mip in (1, 2, 3, 4):
            (healed, slices), (words, samples, count_only, visited) = _per_mip_skips(L, tex, C4_S, mip)
            assert healed == 0 and slices > 0
            print(f"C4 mip {mip}: {words} wave-words absorbed, {samples} of {visited} wave-samples "
                  f"({samples / max(visited, 1):.3f}), {count_only} through the count-only body")
            if mip in (1, 2):
                assert words > 0 and samples > 0, (mip, words, samples)
    finally:
        L.GPU_DestroyTexture(tex)


def test_bright_sun_and_black_channel(gpu, c4_env):
    """A 1e5:1 sun (one 8x8 patch of the environment scaled by 1e5) and an environment whose green channel is 0 everywhere (a lane
    with a zero sum never qualifies): skipping on == off, bit for bit."""
    L = gpu
    env = c4_env.copy()
    env[4, 1000:1008, 1000:1008, :3] *= 1e5
    _on_off(L, env)
    env = c4_env.copy()
    env[..., 1] = 0.0
    _, sk = _on_off(L, env)
    assert sk[0] == 0, sk                                               # every lane has a zero green sum


def test_negative_and_inf_texels(gpu, c4_env):
    """A negative or an infinite texel must switch skipping off for every region that stages it: with one of each in the
    environment the outputs (inf / NaN included) are the same bytes with skipping on and off; with a negative blue channel in
    every texel no region may skip at all."""
    L = gpu
    env = c4_env.copy()
    env[1, 300, 400, 0] = -1e9
    env[3, 1500, 700, 2] = np.inf
    _on_off(L, env)
    env = c4_env.copy()
    env[..., 2] = -np.abs(env[..., 2]) - 1e-3
    _, sk = _on_off(L, env)
    assert sk[:3] == (0, 0, 0), sk


def test_ragged_row_shards_equal_full_dispatch_with_skipping(gpu, c4_env):
    """Rows that are no multiple of the 16-row tile, three shards per face, skipping on: the same bytes as the whole-level dispatch
    (quarter-face regions at 512 -> mip 1, whole-face regions at 4096 -> mip 2)."""
    L = gpu
    L.pbrk_mc_set_absorb(1)
    tex = mc.env_texture(c4_env)
    pipes = L.PBR_MakeIBLPipelines(); arena = L.GPU_MakeDescriptorArena(); g = L.GPU_MakeGraph()
    try:
        for S, mips in ((512, (1,)), (C4_S, (1, 2))):
            maps = pbrhip.PBR_IBLMaps()
            L.PBR_MakeIBLMaps(C.byref(maps), 8, 64, S)
            spec = maps.tex_specular_env_map
            L.PBR_GenPrefilteredEnvMap(tex, spec, 256)
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


def test_tolerance_cut_tables_with_and_without_skipping(gpu, c4_env):
    """GPUX_SetPrefilterTolerance(1e-7) binds shorter tables; the per-word weight bound is taken from the table actually bound, so
    skipping on == off there too."""
    L = gpu
    try:
        L.GPUX_SetPrefilterTolerance(1e-7)
        _on_off(L, c4_env)
    finally:
        L.GPUX_SetPrefilterTolerance(0.0)
