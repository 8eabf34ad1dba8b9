"""CPU checks of what test_gpu_shade_edges.py relies on: the properties of the shade_maps contents, the oracle's `region`, and the
conditioning screen's cap for every frame, seed and flag set the GPU tests compare."""
import numpy as np
import pytest

import shade_maps as SM
from shade_maps import IBL, SHADOWS, SHAFTS


@pytest.mark.parametrize("n", [1, 2, 3, 24, 25, 48, 65])
def test_cube_levels_are_positive_and_tell_texel_face_level_and_channel_apart(n):
    levels = SM.cube_pyramid(n)
    assert [lv.shape for lv in levels] == [(6, m, m, 4) for m in SM.level_sizes(n)] and levels[-1].shape[1] == 1
    for lv in levels:
        assert lv.dtype == np.float32 and (lv[..., 3] == 1).all()
        assert 0.2 < lv[..., :3].min() and lv[..., :3].max() < 4.5
    a = levels[0].astype(np.float64)
    if n >= 48:                    # adjacent texels: the +-2 % checker (4 %) on top of the field's own slope (which falls with n)
        for d in (np.abs(a[:, :, 1:, :3] / a[:, :, :-1, :3] - 1), np.abs(a[:, 1:, :, :3] / a[:, :-1, :, :3] - 1)):
            assert 0.03 < np.median(d) < 0.05 and (d > 0.01).mean() > 0.9, (float(np.median(d)), float((d > 0.01).mean()))
    # the factor alone separates faces, levels and channels by more than 3 % (thousands of tolerances)
    k = np.array([[[SM.factor(f, l, c) for c in range(3)] for l in range(10)] for f in range(6)])
    assert np.abs(k[1:] / k[:-1] - 1).min() > 0.03 and np.abs(k[:, 1:] / k[:, :-1] - 1).min() > 0.03 and np.abs(k[..., 1:] / k[..., :-1] - 1).min() > 0.03
    # other content for the same level (the twins test) differs everywhere
    b = SM.cube_level(n, 0, variant=2)
    assert (np.abs(b[..., :3] / levels[0][..., :3] - 1) > 1e-3).mean() > 0.9


@pytest.mark.parametrize("size", [2, 48, 64, 256])
def test_lut_has_its_own_gradient_in_u_and_in_v(size):
    t = SM.lut(size).astype(np.float64)
    assert t.shape == (size, size, 2) and 0 < t.min() and t.max() < 1
    assert (np.diff(t[..., 0], axis=1) > 0).all() and (np.diff(t[..., 1], axis=0) < 0).all()
    assert np.abs(np.diff(t[..., 0], axis=1)).mean() > 3 * np.abs(np.diff(t[..., 0], axis=0)).mean()
    assert np.abs(np.diff(t[..., 1], axis=0)).mean() > 3 * np.abs(np.diff(t[..., 1], axis=1)).mean()
    assert (SM.lut(size, 1) != SM.lut(size)).any(-1).mean() > 0.9


@pytest.mark.parametrize("sizes", [(48, 24, 48), (50, 25, 50), (520, 520, 64), (1, 1, 2)], ids=lambda s: "x".join(map(str, s)))
def test_oracle_region_is_the_crop_of_the_full_frame(sizes):
    case = SM.ShadeCase(96, 64, *sizes, shadows=True)
    for flags in (IBL, IBL | SHADOWS | SHAFTS):
        full = case.oracle(flags)
        assert np.isfinite(full).all() and (full[..., :3] >= 0).all()
        x0, x1, y0, y1 = region = (3, 70, 2, 41)
        part = case.oracle(flags, region=region)
        assert np.array_equal(part[y0:y1, x0:x1], full[y0:y1, x0:x1])
        part[y0:y1, x0:x1] = 0
        assert (part == 0).all()


def _wild_cases():
    for W, H in SM.RAGGED:
        yield (W, H, 64, 32, 64), SM.FAST_FLAGS + SM.GENERAL_FLAGS
    yield (130, 9, 64, 32, 64), (IBL | SHAFTS, IBL | SHADOWS)
    yield (96, 64, 48, 24, 48), (IBL, IBL | SHADOWS)
    yield (96, 64, 50, 25, 50), (IBL, IBL | SHADOWS)
    yield (96, 64, 520, 520, 64), (IBL,)
    for sizes in ((512, 512, 256), (1, 1, 2), (2, 2, 2)):
        yield (96, 64) + sizes, (IBL, IBL | SHAFTS)
    yield (96, 64, 64, 32, 64), (IBL,)


@pytest.mark.parametrize("shape,flag_sets", list(_wild_cases()), ids=lambda v: "x".join(map(str, v)) if len(v) == 5 else None)
def test_conditioning_screen_stays_under_its_cap(shape, flag_sets):
    """For every wild-byte frame the GPU tests compare (same sizes, seed and flags): the screen removes at most 0.5 % of the surface
    pixels and no sky pixel, the frame has both sky and (beyond one pixel) surface, and shadows darken part of it."""
    case = SM.ShadeCase(*shape, shadows=True)
    if shape[0] * shape[1] > 1:
        assert 0.2 < case.surface.mean() < 0.9                    # surface and sky are both there
    for flags in flag_sets:
        want, keep, share = case.reference(flags)
        assert share <= SM.SCREEN_CAP and keep[~case.surface].all() and keep.mean() >= 0.995
        assert np.isfinite(want).all()
    if shape[0] * shape[1] > 100 and any(f & SHADOWS for f in flag_sets):
        lit, dark = case.oracle(IBL)[..., :3].sum(-1), case.oracle(IBL | SHADOWS)[..., :3].sum(-1)
        assert ((dark < lit * 0.999) & case.surface).mean() > 0.02


def test_screen_removes_only_pixels_that_move_with_the_camera():
    case = SM.ShadeCase(96, 64, 64, 32, 64, seed=0x5EED0E00)
    want, keep, share = case.reference(IBL)
    assert 0 < (~keep).sum() <= 0.005 * case.surface.sum()         # this seed has ill-conditioned pixels, and they are few
    cam = np.array(list(case.glob.camera_pos), np.float32)
    cam[2] = np.nextafter(cam[2], np.float32(np.inf))
    assert SM.rel_map(case.oracle(IBL, camera=cam), want)[keep].max() <= SM.SCREEN_MOVE
