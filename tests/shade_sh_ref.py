"""Reference for K5's SH9 ambient mode (test_sh_shade_cpu.py, test_gpu_shade_sh9.py), built from what the suite already has: the ambient
term enters lighting_pass.glsl:687 linearly, so for one shade_maps.ShadeCase
    F(E) = max(F0 + d * E, 0),   F0 = the oracle's frame with an all-zero irradiance cube,   d = (F1024 - F0) / 1024 = kD * base,
F1024 the oracle's frame with the constant cube 1024 (a power of two: the subtraction's rounding is relative to the ambient term, not
to F0), and E the irradiance of the double contract (sh_ref.irradiance) at the pixel's normal, decoded from its bytes and normalised
in float64.  The oracle itself is not touched.  Also the coefficient sets the tests shade with."""
import numpy as np

import sh_ref
import shade_maps as SM

SH9 = 16                                         # PBRK_SHADE_SH9 == pbrhip.Shade_SH9

# a_i K_i of csrc/sh_shade_core.h: E(n) = sum_i (W_i coef_i) p_i(n), p = {1, y, z, x, xy, yz, 3zz - 1, xz, xx - yy}
_PI = np.pi
K_BASIS = np.array([np.sqrt(1 / (4 * _PI))] + [np.sqrt(3 / (4 * _PI))] * 3 + [np.sqrt(15 / (4 * _PI))] * 2 + [np.sqrt(5 / (16 * _PI))] +
                   [np.sqrt(15 / (4 * _PI)), np.sqrt(15 / (16 * _PI))])
W_FOLD = sh_ref.A_BAND * K_BASIS


def coef_from_weights(w):
    """w [9][3]: the polynomial weights of E per channel -> the 27 SH9 radiance coefficients (float64 [9][3]) that fold to them"""
    return np.asarray(w, np.float64).reshape(9, 3) / W_FOLD[:, None]


def coef_positive():
    """E between 0.3 and 2.6 on the whole sphere, another tint per channel: |band 1| <= 0.45, |band 2| <= 0.25 under a constant >= 1"""
    w = np.zeros((9, 3))
    w[0] = (1.0, 1.3, 1.7)
    w[1] = (0.20, -0.10, 0.15); w[2] = (0.25, 0.30, -0.20); w[3] = (-0.15, 0.20, 0.25)
    w[4] = (0.10, 0.0, -0.10); w[6] = (0.05, -0.05, 0.04); w[8] = (0.0, 0.10, 0.05)
    return coef_from_weights(w)


def coef_partly_negative():
    """E = A + B n.a with |B| > A: negative on the cap around -a (down to about -4), positive elsewhere (up to about 5), plus a little
    band 2.  F0 / d of the wild frames starts at 0.6 and passes 2 at their 5 % quantile, so this is the least that clamps more than
    a handful of their pixels (test_sh_shade_cpu.py counts them); larger magnitudes would only make the pixels where F0 + d E
    crosses zero cancel larger terms, and the criterion's floor (1e-2) is an absolute 1e-6 there."""
    w = np.zeros((9, 3))
    w[0] = (0.45, 0.40, 0.50)
    w[1] = (1.80, -1.50, 0.90); w[2] = (-3.90, -3.60, 4.05); w[3] = (1.20, 1.65, -1.35)
    w[5] = (0.08, 0.0, -0.06); w[6] = (0.04, 0.05, -0.03)
    return coef_from_weights(w)


def coef_random(seed=5):
    return np.random.default_rng(seed).standard_normal((9, 3))


def coef_ringing():
    """strong band 2 over a small constant: E changes sign several times around the sphere"""
    c = np.zeros((9, 3))
    c[0] = (0.5, 0.4, 0.6)
    c[4] = (9.0, -7.0, 5.0); c[5] = (-6.0, 8.0, 7.0); c[6] = (12.0, -10.0, 9.0); c[7] = (5.0, 6.0, -8.0); c[8] = (-7.0, 9.0, 6.0)
    c[2] = (1.0, -1.0, 0.5)
    return c


TINY_NORMALS = ((128, 128, 128), (127, 128, 130), (125, 131, 127), (131, 126, 124))      # |N| = 0.007 .. 0.04


def make_case(W, H, **kw):
    """shade_maps.ShadeCase(W, H, 64, 32, 64, ...) whose wild G-buffer also holds the shortest normals bytes can give: random bytes reach
    |N| > 1.5 on their own, but |N| < 0.1 (all three bytes within 120 .. 135) once in 5000 pixels.  Four surface pixels spread over the
    frame get them (a frame with fewer surface pixels: as many as it has).  Nothing else of the case changes: `surface` depends on
    the depth alone."""
    case = SM.ShadeCase(W, H, 64, 32, 64, **kw)
    if not case.gi:
        ys, xs = np.nonzero(case.surface)
        for j, rgb in enumerate(TINY_NORMALS[:len(ys)]):
            i = (2 * j + 1) * len(ys) // (2 * len(TINY_NORMALS))
            case.gbd["normal"][ys[i], xs[i], :3] = rgb
    return case


def normals(case):
    """the G-buffer's raw normals, float64 [H][W][3]: byte / 255 * 2 - 1 (never the zero vector)"""
    return case.gbd["normal"][..., :3].astype(np.float64) / 255.0 * 2.0 - 1.0


def irradiance_at(coef, n):
    n = np.asarray(n, np.float64)
    return sh_ref.irradiance(coef, n / np.linalg.norm(n, axis=-1, keepdims=True))


class Composite:
    """F0, d and the keep mask of one case and flag set (flags without SH9), computed once; want(coef) is then cheap."""

    def __init__(self, case, flags):
        assert not flags & SH9
        saved = case.irr
        try:
            case.irr, case._ref = np.zeros_like(saved), {}
            self.F0 = case.oracle(flags)
            self.keep, self.share = (np.ones((case.H, case.W), bool), 0.0) if flags & SM.GI else case.screen(flags, self.F0)
            case.irr = np.full_like(saved, 1024.0)
            self.F1024 = case.oracle(flags)
        finally:
            case.irr, case._ref = saved, {}
        self.d = (self.F1024.astype(np.float64) - self.F0.astype(np.float64))[..., :3] / 1024.0
        self.N = normals(case)
        self.case = case

    def want(self, coef=None, E=None):
        """float64 [H][W][4]: max(F0 + d E, 0), alpha as the oracle's.  E: a constant rgb instead of coefficients."""
        E = irradiance_at(coef, self.N) if E is None else np.broadcast_to(np.asarray(E, np.float64), self.N.shape)
        out = self.F0.astype(np.float64).copy()
        out[..., :3] = np.maximum(out[..., :3] + self.d * E, 0.0)
        return out

    def clamped(self, coef):
        """pixels where the final max(out, 0) acts in some channel: F0 + d E < 0"""
        return ((self.F0[..., :3].astype(np.float64) + self.d * irradiance_at(coef, self.N)) < 0.0).any(-1)
