"""Visiting order of the region kernel (k_mc_region.hip, 2e; the 66^2 region shapes): a tile stages the regions of its own face
first, then all the others in index order.  The own face holds a texel's big terms, so every later word is tested for absorption (2c) against a grown sum on
every face, not only on the faces with the lowest index.  Checked here: the order function itself (no GPU), the per-face skip
fractions, the level totals against the index-order loop's figures, and the error against the fp64 oracle."""
import numpy as np
import pytest

import pbrhip
from pbrhip import mc

C4_W, C4_S, C4_MIN = 2048, 4096, 128          # bench C4: 2048^2 environment -> 4096^2 prefiltered cube, Monte-Carlo mips 1..5
REL = 1e-4                                    # the bound of the oracle comparisons of these levels (test_gpu_fullsize.py, bench.py --check)

# wave-samples absorbed by the index-order loop on C4 (profiles/r05_runs.md): the new order must not absorb fewer
INDEX_ORDER_SKIPPED = {2: 374_376_440, 1: 449_714_944}
# Smallest per-face skip fraction over the largest.  In index order (profiles/r06_order.md, step 1) the six faces of mip 2 absorb
# 0.474 0.468 0.428 0.430 0.403 0.431 of their wave-samples (0.850) and those of mip 1 0.790 0.781 0.766 0.773 0.750 0.744 (0.942):
# the faces visited before their neighbours (+-X) lead.  Own face first: 0.474 0.473 0.472 0.475 0.481 0.493 (0.958) and
# 0.790 0.781 0.784 0.793 0.777 0.796 (0.977).  What is left is the level's content per face and the pole of the tangent frame inside
# +-X (more samples flagged for two regions there), not the face index.  The shares sit about halfway between the two measured
# ratios: the counters are deterministic (the sums are), so the margin is for other environments' content only.
MIN_OVER_MAX = {2: 0.93, 1: 0.96}


def test_order_is_a_permutation_starting_with_the_own_face():
    """No GPU: pbrk_mc_region_order is the kernel's own inline (mc_region_visit).  For every face and every G in use (1: whole
    faces; 2: the quarter faces of n = 128; 3, 4: larger sources of the same shape) the visits are a permutation of 0 .. 6 G^2 - 1,
    begin with the own face's regions in index order and go on with the others in index order."""
    L = pbrhip.lib()
    for G in (1, 2, 3, 4):
        GG, NR = G * G, 6 * G * G
        for face in range(6):
            order = [L.pbrk_mc_region_order(face, G, k) for k in range(NR)]
            assert sorted(order) == list(range(NR)), (G, face, order)
            assert order[:GG] == list(range(face * GG, face * GG + GG)), (G, face, order)
            assert order[GG:] == [r for r in range(NR) if r // GG != face], (G, face, order)
        assert L.pbrk_mc_region_order(6, G, 0) == -1 and L.pbrk_mc_region_order(0, G, NR) == -1 and L.pbrk_mc_region_order(0, G, -1) == -1
    assert L.pbrk_mc_region_order(0, 0, 0) == -1


def _dispatch_counters(L, tex, S, mip, f0, f1):
    """Faces [f0, f1) of one level dispatched alone: healed wave-slices, wave-slices, absorbed wave-samples, wave-samples visited."""
    with mc.dispatch_prefilter_units(L, tex, S, [pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, mip, f0, f1, 0, S >> mip, 0.0)]):
        c = mc.counters(L, "region", "skip", "flag")
        return c["healed"], c["slices"], c["abs_samples"], 4 * c["flags"]


@pytest.mark.gpu
def test_skip_fraction_no_longer_follows_the_face_index(gpu, c4_env):
    """C4 mips 2 (whole-face regions) and 1 (quarter faces), every face dispatched alone: see MIN_OVER_MAX."""
    L = gpu
    L.pbrk_mc_set_absorb(1); L.pbrk_mc_set_runs(1)
    tex = mc.env_texture(c4_env)
    try:
        _dispatch_counters(L, tex, C4_S, 2, 0, 1)                      # first launch: allocates the counters
        for mip in (2, 1):
            fr = []
            for f in range(6):
                healed, slices, skipped, visited = _dispatch_counters(L, tex, C4_S, mip, f, f + 1)
                assert healed == 0 and slices > 0 and 0 < skipped <= visited, (mip, f, healed, slices, skipped, visited)
                fr.append(skipped / visited)
            print(f"C4 mip {mip}: skip fraction per face " + " ".join(f"{x:.3f}" for x in fr) + f", min / max {min(fr) / max(fr):.3f}")
            assert min(fr) >= MIN_OVER_MAX[mip] * max(fr), (mip, fr)
    finally:
        L.GPU_DestroyTexture(tex)


@pytest.mark.gpu
def test_level_totals_not_below_index_order(gpu, c4_env):
    """The whole level in one dispatch absorbs at least the wave-samples the index-order loop absorbed (one-sided)."""
    L = gpu
    L.pbrk_mc_set_absorb(1); L.pbrk_mc_set_runs(1)
    tex = mc.env_texture(c4_env)
    try:
        _dispatch_counters(L, tex, C4_S, 2, 0, 1)
        for mip in (2, 1):
            healed, slices, skipped, visited = _dispatch_counters(L, tex, C4_S, mip, 0, 6)
            print(f"C4 mip {mip}: {skipped} of {visited} wave-samples absorbed ({skipped / visited:.3f}); index order: {INDEX_ORDER_SKIPPED[mip]}")
            assert healed == 0 and slices > 0
            assert skipped >= INDEX_ORDER_SKIPPED[mip], (mip, skipped)
    finally:
        L.GPU_DestroyTexture(tex)


@pytest.mark.gpu
def test_rows_against_the_fp64_oracle(gpu, c4_env):
    """A few rows of C4 mips 1 and 2 (faces +X, -Y, +Z, -Z: first, middle and last rows, one next to a face edge) against the fp64
    oracle at the bound the existing oracle comparisons use for these levels; the worst error per level is printed."""
    import pbr_oracle as O
    L = gpu
    L.pbrk_mc_set_absorb(1); L.pbrk_mc_set_runs(1)
    tex = mc.env_texture(c4_env)
    spec = pbrhip.make_texture(pbrhip.Format_RGBA32F, C4_S, C4_S, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps | pbrhip.TextureFlag_StorageImage)
    try:
        L.PBR_GenPrefilteredEnvMap(tex, spec, C4_MIN)
        L.GPU_WaitUntilIdle()
        pyr = O.build_pyramid(c4_env)
        for mip in (1, 2):
            size = C4_S >> mip
            got = pbrhip.read_mip(spec, mip)
            worst = 0.0
            for (f, y) in ((0, 0), (3, size // 2), (4, 1), (5, size - 1)):
                want = O.prefilter_mip(pyr, C4_W, C4_S, mip, faces=(f, f + 1), rows=(y, y + 1))[f, y]
                err = np.abs(got[f, y].astype(np.float64) - want) / np.maximum(np.abs(want), 1e-3)
                worst = max(worst, float(err.max()))
            print(f"C4 mip {mip}: worst relative error against the oracle {worst:.3e}")
            assert worst < REL, (mip, worst)
    finally:
        L.GPU_DestroyTexture(spec)
        L.GPU_DestroyTexture(tex)
