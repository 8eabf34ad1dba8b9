"""K5 (k_shade.hip, k_shade_fast.hip) where the other shade tests never go: ragged frames in every instantiation and both target
formats, column and row ranges through the kernel ABI, cubes that are not powers of two, cubes beyond the cells twin, the fast
kernel at both ends of its range, missing twins, twins after their texture changes, and pbrk_shade's argument checks.

Maps are uploaded as data (shade_maps.py: no precompute kernel runs at a new shape); the device side is gpu_rigs.ShadeRig.  Every
comparison with the oracle is the suite's criterion for K5, rel_err(got[..., :3], want[..., :3], floor=1e-2) < 1e-4 and no NaN, on the
pixels that pass the conditioning screen (ShadeCase.screen: at most 0.5 % of the surface pixels, never a sky pixel; the GI scene is
compared on every pixel).  Bit-equality checks are not screened.  pbrk_shade_last_kernel() says which instantiation ran."""
import numpy as np
import pytest

import shade_maps as SM
from gpu_rigs import ShadeRig
from shade_maps import GI, IBL, SHADOWS, SHAFTS

pytestmark = pytest.mark.gpu

GENERAL, FAST, LIVE = 0, 1, 2


def _fmt(name):
    import pbrhip
    return {"f32": pbrhip.Format_RGBA32F, "f16": pbrhip.Format_RGBA16F}[name]


def check_vs_oracle(case, flags, got, label, region=None):
    """got: the target as read back (float32 or float16 [H][W][4]).  Inside `region` (default: the frame) the screened pixels meet
    the criterion (fp16 targets: at most one code from the oracle's own conversion, alpha 0x3C00).  -> (largest error, screen share)."""
    import pbr_oracle as O
    want, keep, share = case.reference(flags)
    x0, x1, y0, y1 = region if region is not None else (0, case.W, 0, case.H)
    sel = np.zeros((case.H, case.W), bool)
    sel[y0:y1, x0:x1] = True
    sel &= keep
    assert share <= SM.SCREEN_CAP and keep[~case.surface].all()             # at least 99.5 % of the surface pixels and every sky pixel are compared
    if got.dtype == np.float16:
        gb = got.view(np.uint16).astype(np.int32)
        wb = O.f32_to_f16_bits(want).astype(np.int32)
        d = np.abs(gb[..., :3] - wb[..., :3]).max(-1)
        e = int(d[sel].max())
        print(f"{label}: fp16 codes off {e}, screen removed {100 * share:.3f} % of {int(case.surface.sum())} surface pixels")
        assert e <= 1, (label, e, np.argwhere(sel & (d > 1))[:5].tolist())
        assert (gb[y0:y1, x0:x1, 3] == 0x3C00).all(), label
        return e, share
    assert not np.isnan(got).any(), label
    m = SM.rel_map(got, want)
    e = float(m[sel].max())
    print(f"{label}: rel_err {e:.3e}, screen removed {100 * share:.3f} % of {int(case.surface.sum())} surface pixels")
    assert e < SM.REL, (label, e, np.argwhere(sel & (m >= SM.REL))[:5].tolist())
    assert (got[y0:y1, x0:x1, 3] == 1.0).all(), label
    return e, share


# ---- 1. ragged frames, every instantiation, both target formats ----

@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("size", SM.RAGGED, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ragged_frames_fast_and_general_kernel(gpu, size, fmt):
    """Frames of one pixel, under and over one 64 x 4 workgroup and three workgroups wide, wild bytes, cubes 64 / 32 / LUT 64: the
    fast kernel in its four <kIBL, kShafts> instantiations and the general kernel in IBL, sun-only, shafts, IBL + shadows and
    shafts + shadows (a rippled 64^2 sun map), each against the oracle, in an RGBA32F and an RGBA16F target."""
    W, H = size
    case = SM.ShadeCase(W, H, 64, 32, 64, shadows=True)
    rig = ShadeRig(gpu, case, _fmt(fmt))
    try:
        for flags in SM.FAST_FLAGS:
            got = rig.draw_api(flags)
            assert gpu.pbrk_shade_last_kernel() == FAST, flags
            check_vs_oracle(case, flags, got, f"ragged {W}x{H} {fmt} fast flags {flags}")
        gpu.pbrk_shade_set_fast(0)
        for flags in SM.GENERAL_FLAGS:
            got = rig.draw_api(flags)
            assert gpu.pbrk_shade_last_kernel() == GENERAL, flags
            check_vs_oracle(case, flags, got, f"ragged {W}x{H} {fmt} general flags {flags}")
    finally:
        gpu.pbrk_shade_set_fast(-1)
        rig.destroy()


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("size", SM.RAGGED_GI, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ragged_frames_live_shader(gpu, size, fmt):
    """k_shade<true> (8 x 8 pixels per wave, 32 x 8 per workgroup) at widths and heights that are no multiple of 8: the complete live
    shader and IBL + GI on synth_gi_scene, every pixel against the oracle, both target formats."""
    W, H = size
    case = SM.ShadeCase(W, H, 64, 32, 64, gi=True)
    rig = ShadeRig(gpu, case, _fmt(fmt))
    try:
        for flags in SM.GI_FLAGS:
            got = rig.draw_api(flags)
            assert gpu.pbrk_shade_last_kernel() == LIVE, flags
            check_vs_oracle(case, flags, got, f"ragged {W}x{H} {fmt} live flags {flags}")
    finally:
        rig.destroy()


# ---- 2. column and row ranges through the kernel ABI ----

@pytest.mark.parametrize("kernel", ["fast", "general", "live"])
def test_column_and_row_ranges_through_the_kernel_abi(gpu, kernel):
    """PbrkShadeArgs x0 / x1 / y0 / y1: the frame drawn as 4 x 3 rectangles whose cuts fall inside workgroups (and, live: inside 8 x 8
    waves) has the bits of the whole-frame draw; one inner rectangle drawn alone leaves every other pixel at its clear value and
    equals the oracle's `region`."""
    if kernel == "live":
        case, flags, want_kernel = SM.ShadeCase(93, 53, 64, 32, 64, gi=True), SHAFTS | SHADOWS | GI, LIVE
        xs, ys, inner = (0, 7, 8, 33, 93), (0, 3, 52, 53), (7, 33, 5, 41)
    else:
        case = SM.ShadeCase(130, 9, 64, 32, 64, shadows=True)
        flags, want_kernel = ((IBL | SHAFTS, FAST) if kernel == "fast" else (IBL | SHADOWS, GENERAL))
        xs, ys, inner = (0, 1, 64, 65, 130), (0, 3, 8, 9), (3, 70, 2, 7)
    rig = ShadeRig(gpu, case)
    try:
        tw = rig.build_twins()
        rig.clear()
        assert rig.shade_abi(rig.args(flags, tw)) == 0
        assert gpu.pbrk_shade_last_kernel() == want_kernel
        whole = rig.read()
        check_vs_oracle(case, flags, whole, f"ranges {kernel} whole frame")
        rig.clear()
        for j in range(len(ys) - 1):
            for i in range(len(xs) - 1):
                assert rig.shade_abi(rig.args(flags, tw, region=(xs[i], xs[i + 1], ys[j], ys[j + 1]))) == 0
                assert gpu.pbrk_shade_last_kernel() == want_kernel
        assert np.array_equal(rig.read().view(np.uint32), whole.view(np.uint32))
        rig.clear()
        assert rig.shade_abi(rig.args(flags, tw, region=inner)) == 0
        got = rig.read()
        x0, x1, y0, y1 = inner
        outside = np.ones((case.H, case.W), bool)
        outside[y0:y1, x0:x1] = False
        assert (got[outside] == -7.0).all()
        assert np.array_equal(got[y0:y1, x0:x1].view(np.uint32), whole[y0:y1, x0:x1].view(np.uint32))
        part = case.oracle(flags, region=inner)
        want = case.reference(flags)[0]
        assert np.array_equal(part[y0:y1, x0:x1], want[y0:y1, x0:x1]) and (part[outside] == 0).all()
        check_vs_oracle(case, flags, got, f"ranges {kernel} inner rectangle", region=inner)
    finally:
        rig.destroy()


# ---- 3. cubes that are not powers of two ----

def _blended_share(case, lo, hi):
    r4 = case.roughness4[case.surface]
    return float(((r4 > lo) & (r4 < hi)).mean())


@pytest.mark.parametrize("flags", [IBL, IBL | SHADOWS], ids=["ibl", "ibl_shadows"])
@pytest.mark.parametrize("sizes", [(48, 24, 48), (50, 25, 50)], ids=["48", "50"])
def test_cubes_that_are_not_powers_of_two(gpu, sizes, flags):
    """Prefiltered 48 (levels 48, 24, 12, 6, 3, 1), irradiance 24, LUT 48, and 50 / 25 / 50 (50, 25, 12, 6, 3, 1: a level size that is
    odd in the middle of the chain, where W >> l and halving the level above part ways): bordered_level_off, cells_level_off and
    cube_tap_from_st at those sizes; the dispatch must take the general kernel, and every pair of levels is blended by more than
    10 % of the pixels."""
    case = SM.ShadeCase(96, 64, *sizes, shadows=True)
    assert [lv.shape[1] for lv in case.pre_levels] == [sizes[0], sizes[1], 12, 6, 3, 1]
    r4 = case.roughness4[case.surface]
    for lo, hi in ((0, 1), (1, 2), (2, 3)):
        assert _blended_share(case, lo, hi) > 0.10
    assert float(((r4 > 3) & (r4 <= 4)).mean()) > 0.10
    rig = ShadeRig(gpu, case)
    try:
        got = rig.draw_api(flags)
        assert gpu.pbrk_shade_last_kernel() == GENERAL
        check_vs_oracle(case, flags, got, f"cube {sizes[0]} / {sizes[1]} / LUT {sizes[2]} flags {flags}")
    finally:
        rig.destroy()


# ---- 4. beyond the cells twin ----

def test_cubes_beyond_the_cells_twin(gpu):
    """Prefiltered 520: level 0 is sampled from the apron and the other levels from cells (level_fetch with cells_first == 1);
    irradiance 520: no level-0 cells, so fetch_rgb_tap on the apron."""
    case = SM.ShadeCase(96, 64, 520, 520, 64)
    assert _blended_share(case, -1, 1) > 0.10                      # level 0 is really sampled
    rig = ShadeRig(gpu, case)
    try:
        got = rig.draw_api(IBL)
        assert gpu.pbrk_shade_last_kernel() == GENERAL
        check_vs_oracle(case, IBL, got, "cube 520 / 520 / LUT 64 ibl")
    finally:
        rig.destroy()


# ---- 5. the fast kernel at its bounds ----

@pytest.mark.parametrize("sizes", [(512, 512, 256), (1, 1, 2), (2, 2, 2)], ids=lambda s: "x".join(map(str, s)))
def test_fast_kernel_at_its_bounds(gpu, sizes):
    """The largest cubes the fast kernel takes (its fp32 cell index and 32-bit byte offsets are largest there) and the smallest (one
    level, maxl == 0; two levels), IBL and IBL + shafts."""
    case = SM.ShadeCase(96, 64, *sizes)
    rig = ShadeRig(gpu, case)
    try:
        for flags in (IBL, IBL | SHAFTS):
            got = rig.draw_api(flags)
            assert gpu.pbrk_shade_last_kernel() == FAST
            check_vs_oracle(case, flags, got, f"fast kernel, cubes {sizes} flags {flags}")
    finally:
        rig.destroy()


# ---- 6. missing twins through the ABI ----

def test_missing_twins_take_the_general_kernel(gpu):
    """prefiltered_cells, irradiance_cells or lut_cells NULL, each alone and all together: the dispatch takes the general kernel, whose
    no-cells branches (apron taps, lut_fetch on the texture) give the oracle's frame and, to 1e-4, the frame with every twin."""
    case = SM.ShadeCase(96, 64, 64, 32, 64)
    rig = ShadeRig(gpu, case)
    try:
        tw = rig.build_twins()
        assert rig.shade_abi(rig.args(IBL, tw)) == 0 and gpu.pbrk_shade_last_kernel() == FAST
        gpu.pbrk_shade_set_fast(0)
        assert rig.shade_abi(rig.args(IBL, tw)) == 0 and gpu.pbrk_shade_last_kernel() == GENERAL
        gpu.pbrk_shade_set_fast(-1)
        full = rig.read()
        check_vs_oracle(case, IBL, full, "all twins, general kernel")
        for without in (("pre_cells",), ("irr_cells",), ("lut_cells",), ("pre_cells", "irr_cells", "lut_cells")):
            rig.clear()
            assert rig.shade_abi(rig.args(IBL, tw, without=without)) == 0
            assert gpu.pbrk_shade_last_kernel() == GENERAL, without
            got = rig.read()
            check_vs_oracle(case, IBL, got, f"without {'+'.join(without)}")
            e = float(SM.rel_map(got, full).max())
            print(f"without {'+'.join(without)} vs all twins: {e:.3e}")
            assert e < SM.REL, (without, e)
    finally:
        gpu.pbrk_shade_set_fast(-1)
        rig.destroy()


# ---- 7. twins follow their texture ----

@pytest.mark.parametrize("kernel", ["fast", "general"])
def test_twins_follow_their_texture(gpu, kernel):
    """Shade, upload other content into one level of the prefiltered cube, then into the irradiance cube, then into the LUT, and shade
    after each: every frame is the oracle's for the maps as they are then (bordered_valid, cells_valid, lut_cells_valid), and
    differs from the frame before on more than 10 % of the surface pixels."""
    case = SM.ShadeCase(96, 64, 64, 32, 64)
    rig = ShadeRig(gpu, case)
    try:
        gpu.pbrk_shade_set_fast(0 if kernel == "general" else -1)
        prev = rig.draw_api(IBL)
        check_vs_oracle(case, IBL, prev, f"twins {kernel} first frame")
        for which, variant in (("pre1", 2), ("irr", 2), ("lut", 1)):
            rig.upload(which, case.set_maps(which, variant))
            got = rig.draw_api(IBL)
            assert gpu.pbrk_shade_last_kernel() == (GENERAL if kernel == "general" else FAST)
            check_vs_oracle(case, IBL, got, f"twins {kernel} after {which}")
            changed = float((got[..., :3] != prev[..., :3]).any(-1)[case.surface].mean())
            print(f"twins {kernel} after {which}: {100 * changed:.1f} % of the surface pixels changed")
            assert changed > 0.10, (which, changed)
            prev = got
    finally:
        gpu.pbrk_shade_set_fast(-1)
        rig.destroy()


# ---- 8. pbrk_shade's argument checks ----

E_ARG, E_FORMAT = -1, -2
LIVE_FLAGS = SHAFTS | SHADOWS | GI


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _no_prev_level(a):
    a.prev_frame[1] = None


BROKEN = [
    ("width_0", LIVE_FLAGS, _set(width=0), E_ARG), ("height_0", LIVE_FLAGS, _set(height=0), E_ARG),
    ("x_empty", LIVE_FLAGS, _set(x0=5, x1=5), E_ARG), ("x_reversed", LIVE_FLAGS, _set(x0=9, x1=3), E_ARG),
    ("y_empty", LIVE_FLAGS, _set(y0=4, y1=4), E_ARG), ("y_reversed", LIVE_FLAGS, _set(y0=7, y1=2), E_ARG),
    ("x0_negative", LIVE_FLAGS, _set(x0=-1), E_ARG), ("y0_negative", LIVE_FLAGS, _set(y0=-1), E_ARG),
    ("x1_beyond_width", LIVE_FLAGS, _set(x1=38), E_ARG), ("y1_beyond_height", LIVE_FLAGS, _set(y1=14), E_ARG),
    ("no_base_color", LIVE_FLAGS, _set(base_color=None), E_ARG), ("no_normal", LIVE_FLAGS, _set(normal=None), E_ARG),
    ("no_orm", LIVE_FLAGS, _set(orm=None), E_ARG), ("no_emissive", LIVE_FLAGS, _set(emissive=None), E_ARG),
    ("no_depth", LIVE_FLAGS, _set(depth=None), E_ARG), ("no_out", LIVE_FLAGS, _set(out=None), E_ARG),
    ("format_rg16f", LIVE_FLAGS, _set(out_format=1), E_FORMAT), ("format_rgba8", LIVE_FLAGS, _set(out_format=6), E_FORMAT),
    ("no_prefiltered", 0, _set(prefiltered_bordered=None), E_ARG), ("prefiltered_size_0", 0, _set(prefiltered_size=0), E_ARG),
    ("prefiltered_levels_0", 0, _set(prefiltered_levels=0), E_ARG), ("levels_beyond_the_chain", 0, _set(prefiltered_levels=8), E_ARG),
    ("levels_beyond_16", 0, _set(prefiltered_size=1 << 16, prefiltered_levels=17), E_ARG),
    ("ibl_no_irradiance", IBL, _set(irradiance_bordered=None), E_ARG), ("ibl_irradiance_size_0", IBL, _set(irradiance_size=0), E_ARG),
    ("ibl_no_lut", IBL, _set(lut=None), E_ARG), ("ibl_lut_size_0", IBL, _set(lut_size=0), E_ARG),
    ("gi_no_grid", LIVE_FLAGS, _set(lightgrid=None), E_ARG), ("gi_grid_size_0", LIVE_FLAGS, _set(lightgrid_size=0), E_ARG),
    ("gi_grid_size_1025", LIVE_FLAGS, _set(lightgrid_size=1025), E_ARG), ("gi_no_lut", LIVE_FLAGS, _set(lut=None), E_ARG),
    ("gi_no_prev_levels", LIVE_FLAGS, _set(prev_frame_levels=0), E_ARG), ("gi_9_prev_levels", LIVE_FLAGS, _set(prev_frame_levels=9), E_ARG),
    ("gi_prev_w_0", LIVE_FLAGS, _set(prev_frame_w=0), E_ARG), ("gi_prev_h_0", LIVE_FLAGS, _set(prev_frame_h=0), E_ARG),
    ("gi_prev_level_null", LIVE_FLAGS, _no_prev_level, E_ARG),
    ("shadows_no_map", LIVE_FLAGS, _set(sun_depth=None), E_ARG), ("shadows_map_w_0", LIVE_FLAGS, _set(sun_depth_w=0), E_ARG),
    ("shadows_map_h_0", LIVE_FLAGS, _set(sun_depth_h=0), E_ARG), ("shadows_map_too_big", LIVE_FLAGS, _set(sun_depth_w=40000, sun_depth_h=40000), E_ARG),
]


@pytest.fixture(scope="module")
def arg_rig(gpu):
    case = SM.ShadeCase(37, 13, 64, 32, 64, gi=True)
    rig = ShadeRig(gpu, case)
    tw = rig.build_twins()
    rig.clear()
    assert rig.shade_abi(rig.args(IBL, tw)) == 0                  # the unbroken arguments are accepted, in each flag set used below
    assert rig.shade_abi(rig.args(0, tw)) == 0
    assert rig.shade_abi(rig.args(LIVE_FLAGS, tw)) == 0 and gpu.pbrk_shade_last_kernel() == LIVE
    rig.clear()
    yield rig, tw
    rig.destroy()


@pytest.mark.parametrize("name,flags,brk,code", BROKEN, ids=[b[0] for b in BROKEN])
def test_shade_argument_checks(gpu, arg_rig, name, flags, brk, code):
    """Each condition of pbrk_shade's validation block broken in turn, in arguments that are accepted otherwise: the error code comes
    back, nothing is launched (the target keeps its clear value) and pbrk_shade_last_kernel() still names the last successful call."""
    rig, tw = arg_rig
    a = rig.args(flags, tw)
    assert len(a.prev_frame) == 8 and a.prev_frame_levels >= 2 and a.prefiltered_levels == 7
    brk(a)
    assert rig.shade_abi(a) == code
    assert gpu.pbrk_shade_last_kernel() == LIVE
    assert (rig.read() == -7.0).all()


def test_shade_null_arguments(gpu, arg_rig):
    assert gpu.pbrk_shade(None, None) == E_ARG
