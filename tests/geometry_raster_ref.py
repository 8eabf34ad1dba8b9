"""CPU reference of the geometry pass contract, restated in numpy: float64 where the contract says fp64, float32
operations elsewhere, one triangle after the other over the whole frame (no tiles, no bins).  Coverage of a snapped triangle is
the sun pass's rule and is taken from tests/sun_raster_ref.py.

  vertex      clip = M (p, 1) per row as ((m0 x + m1 y) + m2 z) + m3, xy += jitter w; the same with the old matrix and jitter
  reject      vertex index >= vertex count, or a non-finite clip coordinate, or a snapped corner outside +-2^21 px: counted
  clip        only when a corner violates z >= 0, x >= -64 w, x <= 64 w, y >= -64 w, y <= 64 w (Sutherland-Hodgman in that order,
              t = da / (da - db), p = a + t (b - a)); the polygon is drawn as a fan, each fan triangle culled on its own
              (negative area in y-down framebuffer space is drawn)
  interpolate adj = rows (b x c, c x a, a x b) of the corners' (x_c, y_c, w); l = adj (xn, yn, 1); lambda = l / (l0 + l1 + l2); fp64
  depth       (sum lambda z_c) / (sum lambda w), rounded to fp32, kept iff in [0, 1]; LESS; ties: lower triangle; discard before write
  derivatives own centre, horizontal and vertical neighbour of the 2x2 quad; odd minus even
  texture     rho from the uv differences, log2 by log2_poly, clamp, snap 1/256; repeat; texel coordinate snapped to 1/256; lerps
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sun_raster_ref as R  # noqa: E402

f32 = np.float32
FLT_MAX = R.FLT_MAX
LOG2_C = [f32(1.4390145540237427), f32(-0.6799435615539551), f32(0.32559481263160706), f32(-0.08476819097995758)]


def log2_poly(x):
    """log2 of finite float32 x > 1: exponent exactly, degree-4 polynomial on the mantissa; float32 operations in Horner order."""
    x = np.asarray(x, f32)
    b = x.view(np.uint32)
    e = (b >> np.uint32(23)).astype(np.int32) - 127
    t = ((b & np.uint32(0x7FFFFF)) | np.uint32(0x3F800000)).view(f32) - f32(1)
    p = t * (LOG2_C[0] + t * (LOG2_C[1] + t * (LOG2_C[2] + t * LOG2_C[3])))
    return e.astype(f32) + p


def mip_chain(level0):
    """uint8 [h][w][4], power-of-two extents -> list of levels: 2x2 box in fp32 on the decoded values, rint(255 x)."""
    levels = [np.ascontiguousarray(level0, np.uint8)]
    h, w = levels[0].shape[:2]
    assert w & (w - 1) == 0 and h & (h - 1) == 0
    while min(w, h) > 1:
        d = levels[-1].astype(f32) / f32(255)
        s = ((d[0::2, 0::2] + d[0::2, 1::2]) + (d[1::2, 0::2] + d[1::2, 1::2])) * f32(0.25)
        levels.append(np.rint(f32(255) * s).astype(np.uint8))
        h, w = levels[-1].shape[:2]
    return levels


def snap256(x):
    return np.floor(x * f32(256) + f32(0.5)) * f32(1.0 / 256.0)


def lod_of(tex, dxu, dyu):
    """dxu, dyu float32 [n][2] -> (lod float32 [n] snapped to 1/256, nonfinite bool [n])."""
    h, w = tex[0].shape[:2]
    with np.errstate(all="ignore"):
        ax, bx, ay, by = dxu[:, 0] * f32(w), dxu[:, 1] * f32(h), dyu[:, 0] * f32(w), dyu[:, 1] * f32(h)
        lx, ly = ax * ax + bx * bx, ay * ay + by * by
        bad = ~(lx <= FLT_MAX) | ~(ly <= FLT_MAX)
        rho = np.sqrt(np.where(lx > ly, lx, ly))
        big = rho > 1
        lod = np.where(big, log2_poly(np.where(big & ~bad, rho, f32(2))), f32(0)).astype(f32)
    lod = np.minimum(lod, f32(len(tex) - 1))
    return snap256(lod), bad


def bilinear(level, u, v):
    h, w = level.shape[:2]
    uw, vw = u - np.floor(u), v - np.floor(v)
    x, y = snap256(uw * f32(w) - f32(0.5)), snap256(vw * f32(h) - f32(0.5))
    fx, fy = np.floor(x), np.floor(y)
    a, b = (x - fx)[:, None], (y - fy)[:, None]
    i0, j0 = fx.astype(np.int64) % w, fy.astype(np.int64) % h
    i1, j1 = (i0 + 1) % w, (j0 + 1) % h
    d = level.astype(f32) / f32(255)
    c00, c10, c01, c11 = d[j0, i0], d[j0, i1], d[j1, i0], d[j1, i1]
    top, bot = c00 + a * (c10 - c00), c01 + a * (c11 - c01)
    return top + b * (bot - top)


def texture(tex, uv, dxu, dyu):
    """texture() with SAMPLER_LINEAR_WRAP: tex = list of levels, uv / dxu / dyu float32 [n][2] -> float32 [n][4]."""
    lod, bad = lod_of(tex, dxu, dyu)
    with np.errstate(invalid="ignore"):
        bad = bad | ~(np.abs(uv[:, 0]) <= FLT_MAX) | ~(np.abs(uv[:, 1]) <= FLT_MAX)
    u, v = np.where(bad, f32(0), uv[:, 0]), np.where(bad, f32(0), uv[:, 1])
    lod = np.where(bad, f32(len(tex) - 1), lod)
    l0 = lod.astype(np.int64)
    f = (lod - l0.astype(f32))[:, None]
    out = np.zeros((len(u), 4), f32)
    for l in np.unique(l0):
        k = l0 == l
        c0 = bilinear(tex[l], u[k], v[k])
        fk = f[k]
        if (fk > 0).any():
            c1 = bilinear(tex[min(l + 1, len(tex) - 1)], u[k], v[k])
            c0 = np.where(fk > 0, c0 + fk * (c1 - c0), c0)
        out[k] = c0
    return out


def _vertex(m, jit, p):
    x, y, z = f32(p[0]), f32(p[1]), f32(p[2])
    c = [((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] for r in range(4)]
    c[0] = c[0] + jit[0] * c[3]
    c[1] = c[1] + jit[1] * c[3]
    return [f32(v) for v in c]


def _plane(p, c):
    g = f32(64) * c[3]
    return [c[2], g + c[0], g - c[0], g + c[1], g - c[1]][p]


def _snap(c, W, H):
    hw, hh = f32(W * 0.5), f32(H * 0.5)
    xf, yf = hw * (c[0] / c[3]) + hw, hh * (c[1] / c[3]) + hh
    if not (abs(xf) <= R.GUARD) or not (abs(yf) <= R.GUARD):
        return None
    return int(np.rint(xf * f32(256))), int(np.rint(yf * f32(256)))


def setup(draw, v, W, H):
    """One source triangle (v: float32 [3][11]).  Returns None (rejected) or (attr dict or None, list of fan triangles ((X0,Y0),(X1,Y1),(X2,Y2)))."""
    m, mo = np.asarray(draw["m"], f32), np.asarray(draw["m_old"], f32)
    jit, jp = np.asarray(draw["jitter"], f32), np.asarray(draw["jitter_prev"], f32)
    with np.errstate(all="ignore"):
        c = [_vertex(m, jit, v[k]) for k in range(3)]
        o = [_vertex(mo, jp, v[k]) for k in range(3)]
        if not all(abs(x) <= FLT_MAX for ck in c for x in ck):
            return None
        a, b, cc = ([np.float64(ck[0]), np.float64(ck[1]), np.float64(ck[3])] for ck in c)
        cross = lambda p, q: [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]  # noqa: E731
        adj = [cross(b, cc), cross(cc, a), cross(a, b)]
        det = (a[0] * adj[0][0] + a[1] * adj[0][1]) + a[2] * adj[0][2]
        if not det != 0.0:
            return None, []
        all_in = True
        for p in range(5):
            out = sum(not (_plane(p, ck) >= 0) for ck in c)
            if out == 3:
                return None, []
            all_in = all_in and out == 0
        P = [list(ck) for ck in c]
        if not all_in:
            for p in range(5):
                Q = []
                for e in range(len(P)):
                    pa, pb = P[e], P[(e + 1) % len(P)]
                    da, db = _plane(p, pa), _plane(p, pb)
                    ia, ib = bool(da >= 0), bool(db >= 0)
                    if ia and len(Q) < 9:                                 # at most 9 corners per plane, 8 in the end (DESIGN K13 rule 4)
                        Q.append(pa)
                    if ia != ib and len(Q) < 9:
                        t = da / (da - db)
                        Q.append([pa[q] + t * (pb[q] - pa[q]) for q in range(4)])
                P = Q
                if not P:
                    break
            if len(P) < 3:
                return None, []
            P = P[:8]
        S = [_snap(pk, W, H) for pk in P]
        if any(s is None for s in S):
            return None
    fans = []
    for e in range(1, len(S) - 1):
        (x0, y0), (x1, y1), (x2, y2) = S[0], S[e], S[e + 1]
        if (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0) < 0:             # DrawCCW: negative area (y down) is drawn
            fans.append((S[0], S[e], S[e + 1]))
    attr = dict(adj=np.array(adj, np.float64), z=np.array([ck[2] for ck in c], f32), w=np.array([ck[3] for ck in c], f32),
                uv=v[:, 9:11].astype(f32), pos=v[:, 0:3].astype(f32), nrm=v[:, 3:6].astype(f32),
                cs=np.array([[ck[0], ck[1]] for ck in c], f32), old=np.array([[ok[0], ok[1], ok[3]] for ok in o], f32))
    return attr, fans


def coverage(fans, W, H):
    """Linear indices of the pixel centres one source triangle covers (each once): the sun pass's rule per fan triangle."""
    lins = []
    for tri in fans:
        X = np.array([[p[0] for p in tri]], np.int64)
        Y = np.array([[p[1] for p in tri]], np.int64)
        Z = np.full((1, 3), 0.5, f32)
        z0 = np.zeros(1, np.int64)
        lin, _ = R._window(X, Y, Z, z0, z0, z0 + W - 1, z0 + H - 1, W, H, W)
        lins.append(lin)
    return np.unique(np.concatenate(lins)) if lins else np.zeros(0, np.int64)


def lambdas(A, i, j, W, H):
    xn = (2 * i + 1).astype(np.float64) / np.float64(W) - 1.0
    yn = (2 * j + 1).astype(np.float64) / np.float64(H) - 1.0
    with np.errstate(all="ignore"):
        l = [(A["adj"][k, 0] * xn + A["adj"][k, 1] * yn) + A["adj"][k, 2] for k in range(3)]
        s = (l[0] + l[1]) + l[2]
        return [lk / s for lk in l]


def interp(lam, a):
    """a float32 [3] or [3][c] -> float32 [n] or [n][c]."""
    a = np.asarray(a, f32).astype(np.float64)
    with np.errstate(all="ignore"):
        if a.ndim == 1:
            return ((lam[0] * a[0] + lam[1] * a[1]) + lam[2] * a[2]).astype(f32)
        return ((lam[0][:, None] * a[0] + lam[1][:, None] * a[1]) + lam[2][:, None] * a[2]).astype(f32)


def pix(A, i, j, W, H):
    own = lambdas(A, i, j, W, H)
    lx, ly = lambdas(A, i ^ 1, j, W, H), lambdas(A, i, j ^ 1, W, H)
    P = dict(lam=own, uv=interp(own, A["uv"]), pos=interp(own, A["pos"]))
    ox, oy = ((i & 1) == 1)[:, None], ((j & 1) == 1)[:, None]
    with np.errstate(all="ignore"):
        for key, a in (("u", "uv"), ("p", "pos")):
            vx, vy = interp(lx, A[a]), interp(ly, A[a])
            P["dx" + key] = np.where(ox, P[a] - vx, vx - P[a])
            P["dy" + key] = np.where(oy, P[a] - vy, vy - P[a])
    return P


def unorm8(x):
    with np.errstate(invalid="ignore"):
        c = np.where(x >= 0, x, f32(0)).astype(f32)
        c = np.where(c > 1, f32(1), c)
    return np.rint(f32(255) * c).astype(np.uint8)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _normalize(a):
    return a / np.sqrt(_dot(a, a))[:, None]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], 1)


def shade(draw, A, P):
    """geometry_pass.glsl:258-320 for the pixels of P -> base, nrm, orm, emi (uint8 [n][4]), vel (float32 [n][2])."""
    mat = draw["material"]
    n = len(P["uv"])
    with np.errstate(all="ignore"):
        bc = texture(mat[0], P["uv"], P["dxu"], P["dyu"])
        base = unorm8(np.exp2(f32(2.2) * np.log2(bc)).astype(f32))
        orm = unorm8(texture(mat[2], P["uv"], P["dxu"], P["dyu"])); orm[:, 3] = 255
        emi = unorm8(texture(mat[3], P["uv"], P["dxu"], P["dyu"])); emi[:, 3] = 255
        lam = P["lam"]
        N = _normalize(interp(lam, A["nrm"]))
        tn = texture(mat[1], P["uv"], P["dxu"], P["dyu"])
        tsx, tsy = tn[:, 0] * f32(2) - f32(1), tn[:, 1] * f32(2) - f32(1)
        tsz = np.sqrt(f32(1) - (tsx * tsx + tsy * tsy))
        dxu, dyu, dxp, dyp = P["dxu"], P["dyu"], P["dxp"], P["dyp"]
        neg = dxu[:, 0] * dyu[:, 1] - dxu[:, 1] * dyu[:, 0] < 0
        denB = dxp * dyu[:, 0:1] - dyp * dxu[:, 0:1]
        Bn = _normalize(denB - N * _dot(N, denB)[:, None])
        Tn = _cross(Bn, N)
        denT = dxp * dyu[:, 1:2] - dyp * dxu[:, 1:2]
        Tp = _normalize(denT - N * _dot(N, denT)[:, None])
        Bp = _cross(Tp, N)
        T, B = np.where(neg[:, None], Tn, Tp), np.where(neg[:, None], Bn, Bp)
        Nn = (T * tsx[:, None] + B * tsy[:, None]) + N * tsz[:, None]
        nrm = np.concatenate([unorm8(Nn * f32(0.5) + f32(0.5)), np.full((n, 1), 255, np.uint8)], 1)
        cs, cw, old = interp(lam, A["cs"]), interp(lam, A["w"]), interp(lam, A["old"])
        jit, jp = np.asarray(draw["jitter"], f32), np.asarray(draw["jitter_prev"], f32)
        vel = (cs / cw[:, None] - jit) - (old[:, 0:2] / old[:, 2:3] - jp)
    return base, nrm, orm, emi, vel.astype(f32)


def raster(targets, draws):
    """The pass.  targets: dict base / nrm / orm / emi (uint8 [H][W][4]), vel (float16 [H][W][2]), depth (float32 [H][W]); not modified.
    draws: list of dicts m, m_old (float32[16], column-major), jitter, jitter_prev, material (four mip chains), vertices (float32 [n][11]),
    indices (uint32), index_count, first_index, vertex_offset.  Returns (new targets, winner map int32 [H][W] (-1: none), rejected)."""
    H, W = targets["depth"].shape
    out = {k: np.array(v, copy=True) for k, v in targets.items()}
    best = out["depth"].ravel()
    win = np.full(W * H, -1, np.int64)
    attrs, rejected, t = [], 0, 0
    for di, d in enumerate(draws):
        verts, idx = np.asarray(d["vertices"], f32), np.asarray(d["indices"], np.uint32)
        n = int(d["index_count"]) // 3
        assert d["first_index"] + d["index_count"] <= len(idx)
        for k in range(n):
            ix = idx[d["first_index"] + 3 * k:d["first_index"] + 3 * k + 3].astype(np.int64) + int(d["vertex_offset"])
            res = None if (ix >= len(verts)).any() else setup(d, verts[ix], W, H)
            attrs.append(None)
            t += 1
            if res is None:
                rejected += 1
                continue
            A, fans = res
            if not fans:
                continue
            lin = coverage(fans, W, H)
            if not len(lin):
                continue
            A["draw"] = di
            attrs[-1] = A
            i, j = lin % W, lin // W
            lam = lambdas(A, i, j, W, H)
            with np.errstate(all="ignore"):
                num = (lam[0] * np.float64(A["z"][0]) + lam[1] * np.float64(A["z"][1])) + lam[2] * np.float64(A["z"][2])
                den = (lam[0] * np.float64(A["w"][0]) + lam[1] * np.float64(A["w"][1])) + lam[2] * np.float64(A["w"][2])
                z = (num / den).astype(f32)
                ok = (z >= 0) & (z <= 1)
            z = np.where(z == 0, f32(0), z)
            ok &= z < best[lin]                                              # LESS; in submission order, so a tie keeps the lower triangle
            if not ok.any():
                continue
            lin, z, i, j = lin[ok], z[ok], i[ok], j[ok]
            P = pix(A, i, j, W, H)
            alpha = texture(d["material"][0], P["uv"], P["dxu"], P["dyu"])[:, 3]
            keep = ~(alpha < f32(0.3))
            best[lin[keep]] = z[keep]
            win[lin[keep]] = t - 1
    flat = {k: out[k].reshape(W * H, -1) for k in ("base", "nrm", "orm", "emi", "vel")}
    for s in np.unique(win[win >= 0]):
        lin = np.nonzero(win == s)[0]
        A = attrs[s]
        P = pix(A, lin % W, lin // W, W, H)
        base, nrm, orm, emi, vel = shade(draws[A["draw"]], A, P)
        flat["base"][lin], flat["nrm"][lin], flat["orm"][lin], flat["emi"][lin] = base, nrm, orm, emi
        with np.errstate(over="ignore"):
            flat["vel"][lin] = vel.astype(np.float16)
    return out, win.reshape(H, W).astype(np.int32), rejected
