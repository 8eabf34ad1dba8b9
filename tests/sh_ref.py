"""numpy fp64 restatement of csrc/sh_core.h (K17): texel directions and exact solid angles of a cube level, the real SH9 basis
(no Condon-Shortley phase; order 1, y, z, x, xy, yz, 3zz-1, xz, xx-yy), projection and the irradiance in the reference's
E / (2 pi) normalisation.  Everything is vectorised double arithmetic; sums are numpy's pairwise sums."""
import numpy as np

A_BAND = np.array([1 / 2, 1 / 3, 1 / 3, 1 / 3, 1 / 8, 1 / 8, 1 / 8, 1 / 8, 1 / 8])


def corners(n):
    return (2.0 * np.arange(n + 1) - n) / n


def centres(n):
    return (2.0 * np.arange(n) + 1.0 - n) / n


def area(x, y):
    return np.arctan2(x * y, np.sqrt((x * x + y * y) + 1.0))


def solid_angles(n):
    """domega[iy][ix] of an n^2 face (the same on all six)."""
    e = corners(n)
    a = area(e[None, :], e[:, None])                                           # a[iy][ix] = A(e_ix, e_iy)
    return ((a[:-1, :-1] - a[1:, :-1]) - a[:-1, 1:]) + a[1:, 1:]


def directions(n):
    """unit vectors [6][n][n][3] of the texel centres, faces as face_texel_dir of pbr_device.h"""
    c = centres(n)
    sc, tc = np.broadcast_to(c[None, :], (n, n)), np.broadcast_to(c[:, None], (n, n))
    one = np.ones((n, n))
    faces = [(one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one)]
    inv = 1.0 / np.sqrt((sc * sc + tc * tc) + 1.0)
    return np.stack([np.stack([x * inv, y * inv, z * inv], -1) for x, y, z in faces])


def basis(d):
    """d [..., 3] unit vectors -> Y [..., 9]"""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    pi = np.pi
    c0, c1, c2 = np.sqrt(1 / (4 * pi)), np.sqrt(3 / (4 * pi)), np.sqrt(15 / (4 * pi))
    c20, c22 = np.sqrt(5 / (16 * pi)), np.sqrt(15 / (16 * pi))
    return np.stack([c0 * np.ones_like(x), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c20 * (3.0 * (z * z) - 1.0),
                     c2 * (x * z), c22 * (x * x - y * y)], -1)


def project(cube, faces=(0, 6), rows=None):
    """cube float32 [6][n][n][>=3] -> (coef [9][3], S [9][3]) over rows [rows) of faces [faces): coef[k][c] = sum L_c Y_k domega,
    S[k][c] = sum |L_c Y_k domega| (what the tolerances scale with)."""
    cube = np.asarray(cube)
    n = cube.shape[1]
    r0, r1 = (0, n) if rows is None else rows
    f0, f1 = faces
    w = basis(directions(n)[f0:f1, r0:r1]) * solid_angles(n)[None, r0:r1, :, None]     # [f][y][x][9]
    L = cube[f0:f1, r0:r1, :, :3].astype(np.float64)
    terms = w[..., :, None] * L[..., None, :]                                          # [f][y][x][9][3]
    return terms.sum(axis=(0, 1, 2)), np.abs(terms).sum(axis=(0, 1, 2))


def irradiance(coef, where):
    """coef [9][3] (or 27) and either a cube size (-> [6][size][size][3]) or unit vectors [..., 3] (-> [..., 3]); fp64, not rounded"""
    coef = np.asarray(coef, np.float64).reshape(9, 3)
    d = directions(int(where)) if np.ndim(where) == 0 else np.asarray(where, np.float64)
    Y = basis(d)
    out = np.zeros(d.shape[:-1] + (3,))
    for k in range(9):
        out = out + (A_BAND[k] * coef[k]) * Y[..., k, None]
    return out


def irradiance_bound(coef, where):
    """sum_k |a_k coef Y_k| per channel: what one fp32 rounding of the irradiance scales with"""
    coef = np.asarray(coef, np.float64).reshape(9, 3)
    d = directions(int(where)) if np.ndim(where) == 0 else np.asarray(where, np.float64)
    Y = basis(d)
    return sum(np.abs((A_BAND[k] * coef[k]) * Y[..., k, None]) for k in range(9))


def band_limited_cube(n, c):
    """float32 [6][n][n][4]: sum_k c[k][ch] Y_k at the texel centres, alpha 1"""
    c = np.asarray(c, np.float64).reshape(9, 3)
    rgb = np.einsum("fyxk,kc->fyxc", basis(directions(n)), c)
    return np.concatenate([rgb, np.ones((6, n, n, 1))], -1).astype(np.float32)


def hdr_cube(n, seed):
    """the GPU tests' input: rng.random()**8 * 1000 in fp32, one 5e4 texel in a face corner, a few negative texels"""
    rng = np.random.default_rng(seed)
    cube = (rng.random((6, n, n, 4)) ** 8 * 1000.0).astype(np.float32)
    cube[2, 0, n - 1, :3] = 5.0e4
    for f, y, x in ((0, 0, 0), (3, n // 2, n // 3), (5, n - 1, n - 1)):
        cube[f, y, x, :3] = -cube[f, y, x, :3] - np.float32(0.5)
    return cube


def worst_ratio(err, scale):
    """max of err / scale, where a zero scale (a basis function that vanishes at every texel centre used) admits only a zero error"""
    err, scale = np.asarray(err, np.float64), np.asarray(scale, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
    return float(r.max())
