"""Shared reference of the K21 tests (not a test): numpy restatements of csrc/prefilter_ggx_core.h.

  table_f64        the sample table derived independently in numpy fp64 (what GPUX_PrefilterGGXSamples is held to)
  frame / dirs     Nrm, T, B of every texel of a level and the direction of every sample, in separately rounded fp32 with exact fmaf
  colours          per texel and kept sample the trilinear colour c (fp32, panorama_ref's sampler on prebuilt bordered levels)
  prefilter_f64    the criterion of the GPU tests: sum of (double) l.z (double) c over the kept entries, divided by (double) wsum
  prefilter_f32    the contract's own order: one fp32 fmaf chain over the entries, then the fp32 quotient
  quadrature       brute-force fp64 integral of L (n.l) D / integral of (n.l) D for an analytic environment
"""
import numpy as np

import panorama_ref as P

F32 = np.float32


def fmaf(a, b, c):
    """panorama_ref.fmaf, several times faster on big arrays: the product of two fp32 values is exact in double and the double sum is
    rounded once more to fp32; the two roundings can differ from one only where the double sum sits exactly on the midpoint of two
    fp32 values (its low 29 significand bits are 1 0 ... 0), so only those elements -- and anything tiny enough to be subnormal in
    fp32, where the midpoints lie elsewhere -- take the TwoSum route of panorama_ref.fmaf"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        out = s.astype(F32)
        doubt = ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000) | ((np.abs(s) < 2.0 ** -120) & (s != 0)) | ~np.isfinite(s)
    if doubt.any():
        out[doubt] = P.fmaf(a[doubt], b[doubt], c[doubt])
    return out


def lerp_fma(p, q, t):
    p, q, t = np.asarray(p, F32), np.asarray(q, F32), np.asarray(t, F32)
    with np.errstate(all="ignore"):
        return fmaf(t, (q - p).astype(F32), p)


def radical_inverse(i):
    i = np.asarray(i, np.uint64)
    r = np.zeros(i.shape, np.float64)
    for b in range(32):
        r += ((i >> np.uint64(b)) & np.uint64(1)).astype(np.float64) * 2.0 ** -(b + 1)
    return r


def table_f64(roughness, count, src_size, src_levels, lod_bias):
    """-> (kept entries float64 [K][4] of {l.x, l.y, l.z, lod} before rounding, clamped mask [K], kept mask over i [count])"""
    r = float(F32(roughness))
    a2 = (r * r) ** 2
    i = np.arange(count, dtype=np.float64)
    xi1 = (i + 0.5) / count
    phi = 2.0 * np.pi * radical_inverse(np.arange(count))
    c2 = (1.0 - xi1) / (1.0 + (a2 - 1.0) * xi1)
    ct, st = np.sqrt(c2), np.sqrt(1.0 - c2)
    lz = 2.0 * c2 - 1.0
    D = a2 / (np.pi * (c2 * (a2 - 1.0) + 1.0) ** 2)
    raw = 0.5 * np.log2(6.0 * src_size * src_size / (4.0 * np.pi * count * (D / 4.0))) + float(F32(lod_bias))
    lod = np.clip(raw, 0.0, src_levels - 1.0)
    keep = lz.astype(F32) > 0
    e = np.stack([2 * ct * st * np.cos(phi), 2 * ct * st * np.sin(phi), lz, lod], -1)
    return e[keep], (raw <= 0.0)[keep] | (raw >= src_levels - 1.0)[keep], keep


def texel_dirs(size, faces=range(6)):
    """pggx_texel_dir for every texel of the faces: float32 [len(faces)][size][size][3]"""
    n = F32(size)
    c = ((np.arange(size, dtype=F32) + F32(0.5)) / n).astype(F32)
    k = (F32(2) * (c - F32(0.5)).astype(F32)).astype(F32)
    sc, tc = np.meshgrid(k, k)                                                # sc along x, tc along y
    one = np.ones_like(sc)
    table = {0: (one, -tc, -sc), 1: (-one, -tc, sc), 2: (sc, one, tc), 3: (sc, -one, -tc), 4: (sc, -tc, one), 5: (-sc, -tc, -one)}
    r = np.stack([np.stack(table[f], -1) for f in faces]).astype(F32)
    return normalize(r)


def normalize(a):
    a = np.asarray(a, F32)
    x, y, z = a[..., 0], a[..., 1], a[..., 2]
    with np.errstate(all="ignore"):
        ln = np.sqrt((((x * x).astype(F32) + (y * y).astype(F32)).astype(F32) + (z * z).astype(F32)).astype(F32)).astype(F32)
        return (a / ln[..., None]).astype(F32)


def cross(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32))
    def m(p, q):
        return (p * q).astype(F32)
    return np.stack([(m(a[..., 1], b[..., 2]) - m(b[..., 1], a[..., 2])).astype(F32),
                     (m(a[..., 2], b[..., 0]) - m(b[..., 2], a[..., 0])).astype(F32),
                     (m(a[..., 0], b[..., 1]) - m(b[..., 0], a[..., 1])).astype(F32)], -1)


def frame(nrm):
    """-> T, B of pggx_frame, and the mask of texels that took the (1, 0, 0) up vector"""
    nrm = np.asarray(nrm, F32)
    switched = ~(np.abs(nrm[..., 2]) < F32(0.999))
    up = np.where(switched[..., None], np.array([1, 0, 0], F32), np.array([0, 0, 1], F32)).astype(F32)
    T = normalize(cross(up, nrm))
    return T, cross(nrm, T), switched


def dirs(nrm, T, B, entries):
    """d of every texel [...] and entry [K]: float32 [...][K][3]"""
    e = np.asarray(entries, F32)
    n_, t_, b_ = nrm[..., None, :], T[..., None, :], B[..., None, :]
    lx, ly, lz = e[:, 0][:, None], e[:, 1][:, None], e[:, 2][:, None]
    return fmaf(n_, lz, fmaf(b_, ly, (t_ * lx).astype(F32)))


def bordered_levels(levels):
    """[level l as float32 [6][n][n][4]] -> their bordered twins, built once"""
    return [P.bordered(np.asarray(l, F32)) for l in levels]


def sample_bordered(B, d):
    """panorama_ref.sample on a prebuilt bordered twin, RGB only: float32 [..., 3]"""
    n = B.shape[1] - 2
    face, i0, j0, a, b = P.taps(d, n)
    t00, t10 = B[face, j0, i0, :3], B[face, j0, i0 + 1, :3]
    t01, t11 = B[face, j0 + 1, i0, :3], B[face, j0 + 1, i0 + 1, :3]
    a3, b3 = a[..., None], b[..., None]
    return lerp_fma(lerp_fma(t00, t10, a3), lerp_fma(t01, t11, a3), b3)


def colours(bordered, nrm, entries):
    """the trilinear colour of every texel [...] and entry [K]: float32 [...][K][3]"""
    e = np.asarray(entries, F32)
    T, B, _ = frame(nrm)
    top = len(bordered) - 1
    fl = np.floor(e[:, 3])
    f = (e[:, 3] - fl).astype(F32)
    l0 = fl.astype(np.int64)
    l1 = np.minimum(l0 + 1, top)
    out = np.zeros(nrm.shape[:-1] + (len(e), 3), F32)
    for lvl in np.unique(l0):
        sel = np.nonzero(l0 == lvl)[0]
        d = dirs(nrm, T, B, e[sel])
        c0 = sample_bordered(bordered[lvl], d)
        c1 = sample_bordered(bordered[int(l1[sel[0]])], d) if l1[sel[0]] != lvl else c0
        out[..., sel, :] = lerp_fma(c0, c1, f[sel][:, None])
    return out


def prefilter_f64(bordered, nrm, entries, wsum):
    """float64 [...][3]"""
    c = colours(bordered, nrm, entries).astype(np.float64)
    lz = np.asarray(entries, F32)[:, 2].astype(np.float64)
    with np.errstate(all="ignore"):
        return (c * lz[:, None]).sum(axis=-2) / float(wsum)


def prefilter_f32(bordered, nrm, entries, wsum):
    """float32 [...][3]: acc = fmaf(l.z, c, acc) in the order of the entries, then acc / wsum"""
    c = colours(bordered, nrm, entries)
    e = np.asarray(entries, F32)
    acc = np.zeros(nrm.shape[:-1] + (3,), F32)
    for k in range(len(e)):
        acc = fmaf(e[k, 2], c[..., k, :], acc)
    with np.errstate(all="ignore"):
        return (acc / F32(wsum)).astype(F32)


# ---- an analytic environment and the integral the filter estimates ----
def radiance(d):
    """smooth and strictly positive (>= 0.2 on the unit sphere): float64 [..., 3] -> [..., 3]"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([1.0 + 0.6 * x + 0.2 * y * z, 0.8 + 0.5 * z * z - 0.1 * x, 1.2 - 0.7 * y + 0.3 * x * z], -1)


def analytic_levels(n0):
    """radiance at the texel centres of an n0^2 cube (n0 a power of two) and its 2 x 2 box chain: [float32 [6][n][n][4]]"""
    lv = np.ones((6, n0, n0, 4), np.float64)
    lv[..., :3] = radiance(texel_dirs(n0).astype(np.float64))
    out = [lv.astype(F32)]
    while lv.shape[1] > 1:
        lv = 0.25 * (lv[:, 0::2, 0::2] + lv[:, 1::2, 0::2] + lv[:, 0::2, 1::2] + lv[:, 1::2, 1::2])
        out.append(lv.astype(F32))
    return out


def quadrature(nrm, roughness, n_theta=6000, n_phi=192):
    """integral of L(l) (n.l) D(n.h) dl / integral of (n.l) D(n.h) dl over the hemisphere of n, h = normalize(n + l): midpoint rule in
    the polar angle of h (where D varies) and the azimuth; float64 [..., 3]"""
    nrm = np.asarray(nrm, np.float64)
    T, B, _ = frame(nrm.astype(F32))
    T, B = T.astype(np.float64), B.astype(np.float64)
    a2 = float(F32(roughness)) ** 4
    th = (np.arange(n_theta) + 0.5) * (np.pi / 4) / n_theta                   # theta_h in (0, pi / 4): n.l = cos(2 theta_h) > 0
    ph = (np.arange(n_phi) + 0.5) * 2 * np.pi / n_phi
    ch = np.cos(th)
    D = a2 / (np.pi * (ch * ch * (a2 - 1.0) + 1.0) ** 2)
    tl = 2 * th                                                               # polar angle of l; dl = sin(tl) d(tl) dphi = 2 sin(tl) d(th) dphi
    w = np.cos(tl) * D * 2 * np.sin(tl)                                       # per theta: (n.l) D and the measure
    lx = np.sin(tl)[:, None] * np.cos(ph)[None, :]
    ly = np.sin(tl)[:, None] * np.sin(ph)[None, :]
    lz = np.broadcast_to(np.cos(tl)[:, None], lx.shape)
    out = np.zeros(nrm.shape, np.float64)
    for idx in np.ndindex(nrm.shape[:-1]):
        d = lx[..., None] * T[idx] + ly[..., None] * B[idx] + lz[..., None] * nrm[idx]
        L = radiance(d)
        out[idx] = (L * w[:, None, None]).sum(axis=(0, 1)) / (w.sum() * n_phi)
    return out
