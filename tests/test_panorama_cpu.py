"""K20 without a GPU: the reference the GPU tests hold the kernel to (tests/panorama_ref.py) against exact rational arithmetic and
against the CPU oracle, and the host half of the contract -- GPUX_PanoramaDirections -- against numpy fp64 and against K6's formulas."""
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_exact as X  # noqa: E402
import panorama_ref as P  # noqa: E402

# (face size of the sampled level, cube size it is a level of, that level; w x h)
SHAPES = [(1, 8, 3, 7, 5), (2, 8, 2, 37, 19), (3, 12, 2, 64, 32), (8, 8, 0, 32, 16), (8, 8, 0, 130, 3), (8, 8, 0, 1, 1), (8, 8, 0, 5, 1),
          (64, 64, 0, 256, 128)]
EXTENTS = sorted({(w, h) for _, _, _, w, h in SHAPES})
_PYR = {}


def pyramid(W):
    """the oracle's pyramid of a lognormal cube with one 5e4 texel: built once per size, shared, read-only"""
    import pbr_oracle as O
    if W not in _PYR:
        pyr = O.build_pyramid(P.hdr_cube(W, 0x20A0 + W))
        pyr.setflags(write=False)
        _PYR[W] = pyr
    return _PYR[W]


def test_fmaf_emulation_equals_exact_rounding():
    """seeded triples: plain ones, and near-total cancellation (c = -RN(a b) and its neighbours, where the double sum is tiny and the
    second rounding matters most), and products that land on fp32 midpoints"""
    rng = np.random.default_rng(0xF3A)
    n = 1500
    a = rng.normal(0, 1, 3 * n).astype(np.float32) * np.exp2(rng.integers(-20, 20, 3 * n)).astype(np.float32)
    b = rng.normal(0, 1, 3 * n).astype(np.float32)
    c = rng.normal(0, 1, 3 * n).astype(np.float32)
    prod = (a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)
    c[n:2 * n] = -prod[n:2 * n]
    c[2 * n:] = np.nextafter(-prod[2 * n:], np.where(rng.random(n) < 0.5, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    # midpoints: a = 1 + 2^-12, b = 1 + 2^-12 -> a b = 1 + 2^-11 + 2^-24, exactly between two fp32 values once c (a multiple of 2^-23) is added
    am = np.full(64, 1 + 2.0 ** -12, np.float32)
    cm = (rng.integers(-1000, 1000, 64) * 2.0 ** -23).astype(np.float32)
    a, b, c = np.concatenate([a, am]), np.concatenate([b, am]), np.concatenate([c, cm])
    got = P.fmaf(a, b, c)
    bad = 0
    for i in range(len(a)):
        want = X.round_f32(Fr(float(a[i])) * Fr(float(b[i])) + Fr(float(c[i])))
        bad += Fr(float(got[i])) != want
    assert bad == 0, bad


@pytest.mark.parametrize("n,W,level,w,h", SHAPES)
def test_restatement_is_within_the_derived_bound_of_the_oracle(n, W, level, w, h):
    """|restatement - orc_cube_sample| <= 16 * 2^-24 * M per channel, M the largest of that channel's four taps in magnitude.  The two
    differ only in the form of the three lerps (fma against a rounded product and a rounded sum): each lerp's two forms differ by at
    most 8 * 2^-24 * M (|t (q - p)| <= 2 M, three roundings of at most 2^-24 relative each on terms of at most 2 M, and the result's own),
    and the two first-stage differences pass through the convex combination of the second stage as at most one of them."""
    import pbr_oracle as O
    import pbrhip
    pyr = pyramid(W)
    lvl = O.pyramid_level(pyr, W, level)
    assert lvl.shape[1] == n
    dirs = pbrhip.panorama_directions(w, h)
    got, taps = P.sample(lvl, dirs, with_taps=True)
    want = O.cube_sample(pyr, W, dirs.reshape(-1, 3), float(level)).reshape(h, w, 4)
    M = np.abs(taps).max(axis=0).astype(np.float64)
    tol = 16 * 2.0 ** -24 * M
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = float((err / tol).max())
    print(f"n {n} {w}x{h}: worst / tolerance {worst:.4f}; bit-equal {float((got == want).mean()):.3f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("w,h", EXTENTS)
def test_directions_equal_numpy_fp64_to_one_fp32_ulp(w, h):
    """two evaluations each good to under one double ulp, rounded to fp32 values of magnitude at most 1, differ by at most 2^-23"""
    import pbrhip
    got = pbrhip.panorama_directions(w, h)
    assert got.shape == (h, w, 3) and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - P.directions_f64(w, h)).max()
    print(f"{w}x{h}: worst {err:.3e} (bound {2.0 ** -23:.3e})")
    assert err <= 2.0 ** -23, err


@pytest.mark.parametrize("w,h", EXTENTS)
def test_directions_are_the_inverse_of_the_equirect_mapping(w, h):
    """K6's u = atan2(d.y, d.x) / 2 pi + 1/2, v = acos(d.z / |d|) / pi of the returned directions are the pixel centres"""
    import pbrhip
    d = pbrhip.panorama_directions(w, h).astype(np.float64)
    u = np.arctan2(d[..., 1], d[..., 0]) / (2 * np.pi) + 0.5
    v = np.arccos(np.clip(d[..., 2] / np.linalg.norm(d, axis=-1), -1, 1)) / np.pi
    eu = np.abs(u - ((np.arange(w) + 0.5) / w)[None, :])
    eu = np.minimum(eu, 1 - eu)                                      # u wraps
    ev = np.abs(v - ((np.arange(h) + 0.5) / h)[:, None])
    assert eu.max() <= 1e-6 and ev.max() <= 1e-6, (eu.max(), ev.max())


def test_directions_reject_bad_extents():
    import ctypes as C
    import pbrhip
    L = pbrhip.lib()
    buf = (C.c_float * 3)()
    assert L.GPUX_PanoramaDirections(1, 1, buf) == 0
    assert L.GPUX_PanoramaDirections(0, 1, buf) == 1 and L.GPUX_PanoramaDirections(1, 16385, buf) == 1
    assert L.GPUX_PanoramaDirections(1, 1, None) == 1
