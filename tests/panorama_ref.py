"""Shared reference of the K20 tests (not a test): an exact numpy restatement of "given fp32 directions, sample one cube level" as
cube_fetch_rgba<true> of csrc/pbr_device.h does it on the bordered twin of the level -- the face table (major axis by largest
magnitude, ties z, then y, then x), the separately rounded fp32 coordinate ops, the apron (edges through orc_cube_neighbor, corners
((a + b) + c) / 3) and lerp_fma with an exact fmaf, along x and then along y.

The CPU oracle's orc_cube_sample cannot be the bit-exact witness: its lerpf rounds the product and the sum separately where the device
uses one fma, so about 30 % of its values differ from the device's in the last bits (tests/test_panorama_cpu.py bounds the difference).
"""
import ctypes as C

import numpy as np

F32 = np.float32


def fmaf(a, b, c):
    """RN(a * b + c) on float32 arrays with ONE rounding, through doubles: the product of two fp32 values is exact in double; TwoSum
    gives the double sum s and its exact error e; float32(s) is the answer unless s sits exactly on the midpoint of two neighbouring
    fp32 values while e != 0 -- then the exact value lies on e's side of the midpoint."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        cd = c.astype(np.float64)
        s = p + cd
        bb = s - p
        e = (p - (s - bb)) + (cd - bb)                               # TwoSum (Knuth): p + cd == s + e exactly
        f = s.astype(F32)
        r = s - f.astype(np.float64)                                 # exact: what the rounding to fp32 dropped
        g = np.nextafter(f, np.where(r > 0, F32(np.inf), F32(-np.inf)).astype(F32))   # the fp32 neighbour on r's side
        tie = np.isfinite(s) & np.isfinite(g) & (r != 0) & ((f.astype(np.float64) + g.astype(np.float64)) * 0.5 == s)
        # float32(s) resolved the apparent tie to even and took f; with e != 0 there is no tie: the exact value s + e is either short
        # of the midpoint, on f's side (f stands), or past it, on g's side
        away = tie & (e != 0) & ((e > 0) == (r > 0))
        out = np.where(away, g, f)
    return out.astype(F32)


def lerp_fma(p, q, t):
    """pbr_device.h: fmaf(t, q - p, p), the difference rounded to fp32 first"""
    p, q, t = np.asarray(p, F32), np.asarray(q, F32), np.asarray(t, F32)
    with np.errstate(all="ignore"):
        return fmaf(t, (q - p).astype(F32), p)


def bordered(level):
    """float32 [6][n][n][4] -> the bordered twin [6][n + 2][n + 2][4]: interior = the face, edges = the adjacent faces' edge texels
    (orc_cube_neighbor), corners = ((own corner + the edge entry beside it along x) + the one along y) / 3 in fp32"""
    import pbr_oracle as O
    lib = O.lib()
    level = np.ascontiguousarray(level, F32)
    n = level.shape[1]
    assert level.shape == (6, n, n, 4)
    B = np.zeros((6, n + 2, n + 2, 4), F32)
    B[:, 1:-1, 1:-1] = level
    ni, nj = C.c_int(), C.c_int()
    for f in range(6):
        for k in range(n):
            for (i, j) in ((-1, k), (n, k), (k, -1), (k, n)):
                nf = lib.orc_cube_neighbor(f, n, i, j, C.byref(ni), C.byref(nj))
                B[f, j + 1, i + 1] = level[nf, nj.value, ni.value]
        for i in (-1, n):
            for j in (-1, n):
                ci, cj = (0 if i < 0 else n - 1), (0 if j < 0 else n - 1)
                a, b, c = level[f, cj, ci], B[f, cj + 1, i + 1], B[f, j + 1, ci + 1]
                with np.errstate(all="ignore"):
                    B[f, j + 1, i + 1] = (((a + b).astype(F32) + c).astype(F32) / F32(3.0)).astype(F32)
    return B


def select(d):
    """float32 [..., 3] -> face, sc, tc, ma: the Vulkan table, ties z > y > x (v_cubeid / sc / tc / ma_f32)"""
    d = np.asarray(d, F32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    is_z = (az >= ax) & (az >= ay)
    is_y = ~is_z & (ay >= ax)
    is_x = ~is_z & ~is_y
    face = np.where(is_z, np.where(z < 0, 5, 4), np.where(is_y, np.where(y < 0, 3, 2), np.where(x < 0, 1, 0)))
    sc = np.where(is_z, np.where(z < 0, -x, x), np.where(is_y, x, np.where(x < 0, z, -z))).astype(F32)
    tc = np.where(is_z, -y, np.where(is_y, np.where(y < 0, -z, z), -y)).astype(F32)
    ma = np.where(is_z, az, np.where(is_y, ay, ax)).astype(F32)
    assert np.all(is_x | is_y | is_z)
    return face, sc, tc, ma


def taps(d, n):
    """face, i0, j0 (bordered tap coordinates, 0 .. n), a, b (fp32 weights): cube_st_exact and cube_tap_from_st without snap"""
    face, sc, tc, ma = select(d)
    half, nf = F32(0.5), F32(n)
    with np.errstate(all="ignore"):
        s = ((half * sc).astype(F32) / ma).astype(F32) + half
        t = ((half * tc).astype(F32) / ma).astype(F32) + half
        u = ((s * nf).astype(F32) - half).astype(F32)
        v = ((t * nf).astype(F32) - half).astype(F32)
    fu, fv = np.floor(u), np.floor(v)
    i0 = np.clip(fu.astype(np.int64) + 1, 0, n)
    j0 = np.clip(fv.astype(np.int64) + 1, 0, n)
    return face, i0, j0, (u - fu).astype(F32), (v - fv).astype(F32)


def sample(level, dirs, with_taps=False):
    """level float32 [6][n][n][4], dirs float32 [..., 3] -> float32 [..., 4]; with_taps: also the four taps [4][..., 4] (t00, t10, t01, t11)"""
    B = bordered(level)
    n = level.shape[1]
    face, i0, j0, a, b = taps(dirs, n)
    t00, t10 = B[face, j0, i0], B[face, j0, i0 + 1]
    t01, t11 = B[face, j0 + 1, i0], B[face, j0 + 1, i0 + 1]
    a4, b4 = a[..., None], b[..., None]
    out = lerp_fma(lerp_fma(t00, t10, a4), lerp_fma(t01, t11, a4), b4)
    return (out, np.stack([t00, t10, t01, t11])) if with_taps else out


def panorama(level, w, h):
    """what K20 writes into an RGBA32F w x h target from this level: float32 [h][w][4]"""
    import pbrhip
    return sample(level, pbrhip.panorama_directions(w, h))


def directions_f64(w, h):
    """the contract in numpy fp64: float64 [h][w][3]"""
    x, y = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    phi = ((2 * x + 1) / w - 1) * np.pi
    theta = (2 * y + 1) / (2 * h) * np.pi
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    return np.stack([st * np.cos(phi)[None, :], st * np.sin(phi)[None, :], np.broadcast_to(ct, (h, w))], -1)


def hdr_cube(n, seed, sun=True):
    """a lognormal RGBA cube level 0 with one 5e4 texel: float32 [6][n][n][4]"""
    rng = np.random.default_rng(seed)
    c = np.exp(rng.normal(0.0, 1.5, (6, n, n, 4))).astype(F32)
    if sun:
        c[int(rng.integers(6)), int(rng.integers(n)), int(rng.integers(n)), :3] = F32(5.0e4)
    return c
