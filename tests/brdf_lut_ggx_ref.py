"""Shared reference of the K22 tests (not a test): numpy restatements of csrc/brdf_lut_ggx_core.h.

  table_f64    the sample table derived independently in numpy fp64 (what GPUX_BrdfLutGGXSamples is held to)
  coords       (i + 1/2) / n in fp32: N.V of a column, the roughness of a row
  terms        the per-sample fp32 terms tA, tB of every (row, column, sample), bit for bit: separately rounded fp32, exact fmaf
  lut_f64      the criterion of the GPU tests: the fp64 sum of a texel's terms divided by N
  integral     the independent fp64 integral over light directions, D evaluated explicitly (no pdf, no Jacobian of the sampling)
"""
import numpy as np

from prefilter_ggx_ref import F32, fmaf, radical_inverse

SCHLICK, CORRELATED = 0, 1


def table_f64(count):
    """float64 [count][3] of {xi1, cos phi, sin phi} before rounding"""
    i = np.arange(count, dtype=np.float64)
    phi = 2.0 * np.pi * radical_inverse(np.arange(count))
    return np.stack([(i + 0.5) / count, np.cos(phi), np.sin(phi)], -1)


def coords(n, idx=None):
    idx = np.arange(n) if idx is None else np.asarray(idx)
    return ((idx.astype(F32) + F32(0.5)) / F32(n)).astype(F32)


def terms(nv, r, table, visibility):
    """nv float32 [C], r float32 [R], table float32 [N][3] -> (tA, tB) float32 [R][C][N], the contract's expressions in its order"""
    one, zero = F32(1), F32(0)
    nv = np.asarray(nv, F32)[None, :, None]
    r = np.asarray(r, F32)[:, None, None]
    xi1 = np.asarray(table, F32)[None, None, :, 0]
    cphi = np.asarray(table, F32)[None, None, :, 1]
    with np.errstate(all="ignore"):
        a = (r * r).astype(F32)
        a2 = (a * a).astype(F32)
        c2 = ((one - xi1) / (one + ((a2 - one) * xi1).astype(F32)).astype(F32)).astype(F32)
        hz = np.sqrt(c2).astype(F32)
        hx = (np.sqrt((one - c2).astype(F32)).astype(F32) * cphi).astype(F32)
        hz2 = (hz + hz).astype(F32)
        rhz = (one / hz).astype(F32)
        vx = np.sqrt((one - (nv * nv).astype(F32)).astype(F32)).astype(F32)
        vh = fmaf(vx, hx, (nv * hz).astype(F32))
        lz = fmaf(vh, hz2, -nv)
        q = np.maximum((one - vh).astype(F32), zero)
        q2 = (q * q).astype(F32)
        fc = ((q2 * q2).astype(F32) * q).astype(F32)
        num = ((vh * rhz).astype(F32) * lz).astype(F32)
        if visibility == SCHLICK:
            k = (a * F32(0.5)).astype(F32)
            omk = (one - k).astype(F32)
            cv = (one / fmaf(nv, omk, k)).astype(F32)
            gv = ((num * cv).astype(F32) / fmaf(lz, omk, k)).astype(F32)
        else:
            oma2 = (one - a2).astype(F32)
            sv = np.sqrt(fmaf((nv * nv).astype(F32), oma2, a2)).astype(F32)
            sl = np.sqrt(fmaf((lz * lz).astype(F32), oma2, a2)).astype(F32)
            gv = ((num + num).astype(F32) / fmaf(lz, sv, (nv * sl).astype(F32))).astype(F32)
        gv = np.where((lz > 0) & (vh > 0), gv, zero).astype(F32)
        return (gv * (one - fc).astype(F32)).astype(F32), (gv * fc).astype(F32)


def lut_f64(w, h, table, visibility, rows=None):
    """float64 [rows][w][2]: per texel the fp64 sum of its fp32 terms, divided by N; row by row to bound the temporaries"""
    rows = range(h) if rows is None else rows
    nv = coords(w)
    out = np.zeros((len(rows), w, 2), np.float64)
    for j, y in enumerate(rows):
        tA, tB = terms(nv, coords(h, [y]), table, visibility)
        out[j, :, 0] = tA[0].astype(np.float64).sum(-1) / len(table)
        out[j, :, 1] = tB[0].astype(np.float64).sum(-1) / len(table)
    return out


# ---- the integral the table estimates ----
def _panels(lo, hi, peak, width, levels):
    """break points of [lo, hi] graded geometrically towards `peak`: peak +- width 2^j, j = 0 .. levels - 1, clipped"""
    pts = {lo, hi}
    if lo < peak < hi:
        pts.add(peak)
    for j in range(levels):
        for s in (-1.0, 1.0):
            p = peak + s * width * 2.0 ** j
            if lo < p < hi:
                pts.add(p)
    return np.array(sorted(pts))


def _rule(breaks, order):
    """composite Gauss-Legendre nodes and weights on the panels between `breaks`"""
    x, w = np.polynomial.legendre.leggauss(order)
    lo, hi = breaks[:-1, None], breaks[1:, None]
    return (0.5 * (hi + lo) + 0.5 * (hi - lo) * x[None, :]).ravel(), (0.5 * (hi - lo) * w[None, :]).ravel()


def integral(nv, r, visibility, order=24):
    """(A, B) in fp64 for one (N.V, roughness): the integral over the upper hemisphere of light directions L, in solid angle, of
    D(N.H) G (1 - Fc) / (4 N.V) and of D(N.H) G Fc / (4 N.V), H = normalize(L + V).  D is the GGX density itself; nothing of the
    importance sampling (its pdf, the Jacobian 4 V.H) enters.  The rule is in L: polar angle and azimuth of L, composite
    Gauss-Legendre of `order` nodes on panels graded geometrically towards the mirror direction (polar angle of V, azimuth pi),
    where D peaks with an angular width of about 2 a; the integrand is analytic inside every panel, and even in the azimuth, so
    half of it is integrated and doubled."""
    nv, r = float(nv), float(r)
    a = r * r
    a2 = a * a
    tv = np.arccos(nv)
    vx = np.sqrt(1.0 - nv * nv)
    # the lobe's width as an azimuth: an angle of 2 a seen at polar angle tv; near the pole every azimuth is close
    wphi = min(np.pi, 2.0 * a / max(np.sin(tv), 1e-3))
    th, wth = _rule(_panels(0.0, 0.5 * np.pi, tv, 0.5 * a, 12), order)
    ph, wph = _rule(_panels(0.0, np.pi, np.pi, 0.5 * wphi, 12), order)
    st, ct = np.sin(th)[:, None], np.cos(th)[:, None]
    lx, ly, lz = st * np.cos(ph)[None, :], st * np.sin(ph)[None, :], np.broadcast_to(ct, (len(th), len(ph)))
    hx, hy, hz = lx + vx, ly, lz + nv
    ln = np.sqrt(hx * hx + hy * hy + hz * hz)
    nh, vh = hz / ln, (vx * hx + nv * hz) / ln
    D = a2 / (np.pi * (nh * nh * (a2 - 1.0) + 1.0) ** 2)
    if visibility == SCHLICK:
        k = 0.5 * a
        G = (nv / (nv * (1.0 - k) + k)) * (lz / (lz * (1.0 - k) + k))
        f = D * G / (4.0 * nv)
    else:
        vis = 0.5 / (lz * np.sqrt(nv * nv * (1.0 - a2) + a2) + nv * np.sqrt(lz * lz * (1.0 - a2) + a2))
        f = D * vis * lz                                                       # G / (4 N.V N.L) = Vis
    fc = (1.0 - vh) ** 5
    wgt = 2.0 * (wth * np.sin(th))[:, None] * wph[None, :]
    return float((f * (1.0 - fc) * wgt).sum()), float((f * fc * wgt).sum())
