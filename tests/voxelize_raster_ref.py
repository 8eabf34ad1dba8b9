"""CPU reference of the voxelise pass contract, restated in numpy per triangle over its pixel box: no bins, no keys.
Fragments are applied in (triangle, pixel row, pixel column) order and the last one to address a voxel owns it; the owners are then
shaded.  float64 where the contract says fp64, float32 operations elsewhere.  texture(), snap256 and the shadow tap's conventions
are those of tests/geometry_raster_ref.py and tests/sun_raster_ref.py, by import.

  vertex      v_k = SSBO1[base + k]; p_k = SSBO0[11 v_k + 0..2]; a position past the end of SSBO0 or a non-finite one: rejected, counted;
              uv_k = SSBO0[11 (base + k) + 9, + 10] (the shader's quirk: vertex number gl_VertexIndex), 0 past the end
  axis        n = cross(p1 - p0, p2 - p0); m = max(max(|n.x|, |n.y|), |n.z|) with max(x, y) = y if x < y else x; m == |n.x|: yzx,
              else m == |n.y|: zxy, else xyz
  snap        g = p * scale; xf = (N/2) x + N/2; a non-finite xf, yf or z * 0.5 + 0.5, or |xf|, |yf| > 2^21: rejected, counted;
              X = rint(256 xf); zero area: nothing
  coverage    pixel (i, j) iff the closed square [256 i, 256 i + 256]^2 meets the closed triangle: the bounding boxes overlap and, for each
              edge with the inside positive, the largest of the four corner values is >= 0 (exact integers)
  interpolate a = a0 + (E1 (a1 - a0) + E2 (a2 - a0)) / area at the pixel centre, fp64, rounded once; uv derivatives in 2 x 2 quads
  fragment    coord = trunc((ndc * 0.5 + 0.5) * N), kept iff -1 < the product < N on every axis; value = emissive + ((shadow base) LdotN) sun
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_raster_ref as G  # noqa: E402
import sun_raster_ref as R  # noqa: E402

f32 = np.float32
SUN_EMISSION = np.array([f32(5), f32(5) * f32(0.9), f32(5) * f32(0.7)], f32)
SHADOW_PX = f32(1.0 / 2048.0)


def shadow_sample(depth, u, v, ref):
    """sampler2DShadow, linear / clamp / Less, coordinates snapped to 1/256 texel: depth float32 [h][w]; u, v, ref float32 [n]."""
    h, w = depth.shape
    with np.errstate(all="ignore"):
        fx, fy = G.snap256(u * f32(w) - f32(0.5)), G.snap256(v * f32(h) - f32(0.5))
        flx, fly = np.floor(fx), np.floor(fy)
        a, b = fx - flx, fy - fly
        i0 = np.fmin(np.fmax(flx, f32(-1)), f32(w)).astype(np.int64)
        j0 = np.fmin(np.fmax(fly, f32(-1)), f32(h)).astype(np.int64)
        i1, j1 = np.clip(i0 + 1, 0, w - 1), np.clip(j0 + 1, 0, h - 1)
        i0, j0 = np.clip(i0, 0, w - 1), np.clip(j0, 0, h - 1)
        c = [(ref < depth[jj, ii]).astype(f32) for jj, ii in ((j0, i0), (j0, i1), (j1, i0), (j1, i1))]
        top, bot = c[0] + a * (c[1] - c[0]), c[2] + a * (c[3] - c[2])
        return (top + b * (bot - top)).astype(f32)


def _max(x, y):
    return y if x < y else x


def setup(draw, local_tri, N):
    """One triangle of a draw.  Returns None (rejected) or a dict, or False (nothing drawn)."""
    v, ix = draw["vertices"], draw["indices"]
    nf = len(v)
    base = int(draw["first_vertex"]) + 3 * local_tri
    p, uv = np.zeros((3, 3), f32), np.zeros((3, 2), f32)
    for k in range(3):
        o = 11 * int(ix[base + k])
        if o + 2 >= nf:
            return None
        p[k] = v[o:o + 3]
        if not np.isfinite(p[k]).all():
            return None
        u = (base + k) * 11 + 9
        uv[k, 0] = v[u] if u < nf else 0
        uv[k, 1] = v[u + 1] if u + 1 < nf else 0
    scale = f32(draw["scale"])
    with np.errstate(all="ignore"):
        e1, e2 = p[1] - p[0], p[2] - p[0]
        n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], f32)
        ab = np.abs(n)
        m = _max(_max(ab[0], ab[1]), ab[2])
        axis = 0 if m == ab[0] else (1 if m == ab[1] else 2)
        g = p * scale
        sw = g[:, [1, 2, 0]] if axis == 0 else (g[:, [2, 0, 1]] if axis == 1 else g)
        hn = f32(N * 0.5)
        xf, yf, z = hn * sw[:, 0] + hn, hn * sw[:, 1] + hn, sw[:, 2] * f32(0.5) + f32(0.5)
        if not ((np.abs(xf) <= R.GUARD).all() and (np.abs(yf) <= R.GUARD).all() and np.isfinite(z).all()):
            return None
        X, Y = np.rint(xf * f32(256)).astype(np.int64), np.rint(yf * f32(256)).astype(np.int64)
        area = int((X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]))
        if area == 0:
            return False
        nn = n / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    i0, i1 = max(-((256 - int(X.min())) // 256), 0), min(int(X.max()) // 256, N - 1)      # 256 i + 256 >= min, 256 i <= max
    j0, j1 = max(-((256 - int(Y.min())) // 256), 0), min(int(Y.max()) // 256, N - 1)
    if i0 > i1 or j0 > j1:
        return False
    return dict(X=X, Y=Y, area=area, p=p, uv=uv, n=nn.astype(f32), g=g.astype(f32), axis=axis, box=(i0, j0, i1, j1))


def coverage(T):
    """Pixels (i, j) of the box that produce a fragment, in (j, i) order."""
    i0, j0, i1, j1 = T["box"]
    j, i = np.meshgrid(np.arange(j0, j1 + 1, dtype=np.int64), np.arange(i0, i1 + 1, dtype=np.int64), indexing="ij")
    i, j = i.ravel(), j.ravel()
    X, Y = T["X"], T["Y"]
    s = 1 if T["area"] > 0 else -1
    cov = np.ones(len(i), bool)
    for a, b in ((1, 2), (2, 0), (0, 1)):
        best = None
        for cx in (0, 256):
            for cy in (0, 256):
                e = s * ((X[b] - X[a]) * (256 * j + cy - Y[a]) - (Y[b] - Y[a]) * (256 * i + cx - X[a]))
                best = e if best is None else np.maximum(best, e)
        cov &= best >= 0
    return i[cov], j[cov]


def edges(T, i, j):
    X, Y = T["X"], T["Y"]
    Px, Py = 256 * i + 128, 256 * j + 128
    E1 = (X[0] - X[2]) * (Py - Y[2]) - (Y[0] - Y[2]) * (Px - X[2])
    E2 = (X[1] - X[0]) * (Py - Y[0]) - (Y[1] - Y[0]) * (Px - X[0])
    return E1.astype(np.float64), E2.astype(np.float64)


def interp(T, E, a):
    """a float32 [3][c] -> float32 [n][c]."""
    a = np.asarray(a, f32).astype(np.float64)
    inv = 1.0 / np.float64(T["area"])
    with np.errstate(all="ignore"):
        return (a[0] + (E[0][:, None] * (a[1] - a[0]) + E[1][:, None] * (a[2] - a[0])) * inv).astype(f32)


def coords(T, i, j, N):
    """Voxel coordinates of the fragments and which of them are kept."""
    with np.errstate(all="ignore"):
        q = (interp(T, edges(T, i, j), T["g"]) * f32(0.5) + f32(0.5)) * f32(N)
        keep = ((q > f32(-1)) & (q < f32(N))).all(1)
    c = np.where(keep[:, None], q, 0).astype(np.int64)                    # astype truncates toward zero
    return c, keep


def shade(draw, sun_map, T, i, j):
    """rgb float32 [n][3] of the fragments at pixels (i, j) of one triangle."""
    own = edges(T, i, j)
    ws, uv = interp(T, own, T["p"]), interp(T, own, T["uv"])
    ux, uy = interp(T, edges(T, i ^ 1, j), T["uv"]), interp(T, edges(T, i, j ^ 1), T["uv"])
    ox, oy = ((i & 1) == 1)[:, None], ((j & 1) == 1)[:, None]
    with np.errstate(all="ignore"):
        dxu, dyu = np.where(ox, uv - ux, ux - uv), np.where(oy, uv - uy, uy - uv)
        m = np.asarray(draw["sun"], f32)
        s = [((m[r] * ws[:, 0] + m[4 + r] * ws[:, 1]) + m[8 + r] * ws[:, 2]) + m[12 + r] for r in range(3)]
        su, sv, sz = (s[0] * f32(0.5) + f32(0.5)) + SHADOW_PX, (s[1] * f32(0.5) + f32(0.5)) + SHADOW_PX, s[2] - f32(0.001)
        shadow = shadow_sample(sun_map, su, sv, sz)
        L = -np.asarray(draw["sun_dir"], f32)[:3]
        d = (L[0] * T["n"][0] + L[1] * T["n"][1]) + L[2] * T["n"][2]
        ldn = f32(0) if d < 0 else d
        bc = G.texture(draw["material"][0], uv, dxu, dyu)[:, :3]
        em = G.texture(draw["material"][1], uv, dxu, dyu)[:, :3]
        return (em + ((shadow[:, None] * bc) * ldn) * SUN_EMISSION).astype(f32)


def voxelize(grid, sun_map, draws, N):
    """The pass on `grid` (float16 [N][N][N][4], not modified).  draws: dicts with vertices (float32, flat: SSBO0), indices (uint32: SSBO1),
    vertex_count, instance_count, first_vertex, scale, sun (float32[16], column-major), sun_dir (3 or 4 floats), material = (base colour
    chain, emissive chain).  Returns (new grid, info): info has the owner of every voxel (tri, i, j: int64 [N^3], -1 = nobody), the axis
    of every triangle (-1: not drawn), the number of fragments kept, hits (triangles that addressed each voxel), the number of contested
    voxels, and the rejected count."""
    grid = np.asarray(grid, np.float16)
    assert grid.shape == (N, N, N, 4)
    sun_map = np.asarray(sun_map, f32)
    own_t, own_i, own_j = (np.full(N ** 3, -1, np.int64) for _ in range(3))
    hits = np.zeros(N ** 3, np.int64)
    tris, axes, rejected, frags, trunc0 = [], [], 0, 0, 0
    for di, d in enumerate(draws):
        n = int(d["vertex_count"]) // 3
        if n == 0 or d["instance_count"] == 0:
            continue
        assert d["first_vertex"] + d["vertex_count"] <= len(d["indices"])
        for k in range(n):
            T = setup(d, k, N)
            t = len(tris)
            tris.append(None)
            axes.append(-1)
            if T is None:
                rejected += 1
                continue
            if T is False:
                continue
            T["draw"] = di
            i, j = coverage(T)
            if not len(i):
                continue
            c, keep = coords(T, i, j, N)
            i, j, c = i[keep], j[keep], c[keep]
            if not len(i):
                continue
            tris[t], axes[t] = T, T["axis"]
            with np.errstate(all="ignore"):
                q = (interp(T, edges(T, i, j), T["g"]) * f32(0.5) + f32(0.5)) * f32(N)
            trunc0 += int((q < 0).any(1).sum())
            lin = (c[:, 2] * N + c[:, 1]) * N + c[:, 0]
            frags += len(lin)
            np.add.at(hits, np.unique(lin), 1)
            own_t[lin], own_i[lin], own_j[lin] = t, i, j                    # in (j, i) order: the last fragment of a voxel stays
    out = grid.copy().reshape(N ** 3, 4)
    for t in np.unique(own_t[own_t >= 0]):
        lin = np.nonzero(own_t == t)[0]
        T = tris[t]
        rgb = shade(draws[T["draw"]], sun_map, T, own_i[lin], own_j[lin])
        with np.errstate(over="ignore"):
            out[lin, :3] = rgb.astype(np.float16)
        out[lin, 3] = 1
    info = dict(tri=own_t, i=own_i, j=own_j, axes=np.array(axes, np.int64), fragments=frags, contested=int((hits > 1).sum()),
                truncated_to_zero=trunc0, rejected=rejected, tris=tris, hits=hits)
    return out.reshape(N, N, N, 4), info
