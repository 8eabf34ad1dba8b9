"""CPU reference of the sun depth pass contract, restated per triangle over its pixel box in numpy.

It follows the stated rules, not the HIP kernel's structure (no tiles, no bins):
  transform   clip = M (p, 1) in fp32, each row as ((m0 x + m1 y) + m2 z) + m3, then divided by w (correctly rounded fp32);
              xf = (W/2) xd + W/2, yf = (H/2) yd + H/2, depth zd
  reject      a vertex index >= the vertex count, a non-finite xf / yf / zd, or |xf| / |yf| > 2^21 px: not drawn, counted
  snap        X = rint(256 xf), Y = rint(256 yf) (1/256 px, ties to even)
  coverage    pixel (i, j) has its centre at (256 i + 128, 256 j + 128); E0, E1, E2 = edge functions of the edges v1->v2, v2->v0,
              v0->v1 (edge(a->b, p) = (b.x-a.x)(p.y-a.y) - (b.y-a.y)(p.x-a.x)) in exact integers; both windings are drawn, signs taken
              so that the inside is positive; a centre exactly on an edge is covered only for a top edge (horizontal, inside below,
              y down) or a left edge (inside to the right); zero area draws nothing
  depth       inv = 1 / (E0 + E1 + E2) and z = z0 + (E1 (z1 - z0) + E2 (z2 - z0)) inv in fp64, rounded to fp32; kept iff 0 <= z <= 1;
              -0 becomes +0; the target keeps min(target, every kept fragment) (LESS test + write)
"""
import numpy as np

GUARD = 2.0 ** 21
FLT_MAX = np.float32(3.4028234663852886e38)


def pixel_matrix(W, H, w=1.0):
    """Column-major float32[16] that maps (x, y, z) in framebuffer pixels to clip space with clip.w = w (ortho: last row (0,0,0,w))."""
    M = np.zeros((4, 4), np.float64)
    M[0, 0], M[0, 3] = 2.0 / W * w, -1.0 * w
    M[1, 1], M[1, 3] = 2.0 / H * w, -1.0 * w
    M[2, 2] = w
    M[3, 3] = w
    return M.T.astype(np.float32).ravel()


def transform(pos, M, W, H):
    """pos float32 [n][3], M column-major float32[16] -> xf, yf, zd (float32 [n])."""
    m = np.asarray(M, np.float32).ravel()
    pos = np.asarray(pos, np.float32)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    with np.errstate(all="ignore"):
        c = [((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] for r in range(4)]
        xd, yd, zd = c[0] / c[3], c[1] / c[3], c[2] / c[3]
        hw, hh = np.float32(W * 0.5), np.float32(H * 0.5)
        xf = hw * xd + hw
        yf = hh * yd + hh
    return xf.astype(np.float32), yf.astype(np.float32), zd.astype(np.float32)


def assemble(pos, indices, draws, W, H):
    """draws: [(index_count, instance_count, first_index, vertex_offset, M)] -> (X, Y int64 [n][3], Z float32 [n][3], rejected)."""
    pos = np.asarray(pos, np.float32)
    indices = np.asarray(indices, np.uint32)
    nv = len(pos)
    Xs, Ys, Zs, rejected = [], [], [], 0
    for index_count, instance_count, first_index, vertex_offset, M in draws:
        n = int(index_count) // 3
        if n == 0 or instance_count == 0:
            continue
        assert first_index + index_count <= len(indices)
        ix = indices[first_index:first_index + 3 * n].astype(np.int64).reshape(n, 3) + int(vertex_offset)
        bad = (ix >= nv).any(1)
        rejected += int(bad.sum())
        ix = ix[~bad]
        xf, yf, zd = transform(pos[ix.ravel()], M, W, H)
        xf, yf, zd = xf.reshape(-1, 3), yf.reshape(-1, 3), zd.reshape(-1, 3)
        with np.errstate(invalid="ignore"):
            ok = ((np.abs(xf) <= GUARD) & (np.abs(yf) <= GUARD) & (np.abs(zd) <= FLT_MAX)).all(1)
        rejected += int((~ok).sum())
        Xs.append(np.rint(xf[ok] * np.float32(256)).astype(np.int64))
        Ys.append(np.rint(yf[ok] * np.float32(256)).astype(np.int64))
        Zs.append(zd[ok])
    if not Xs:
        e = np.zeros((0, 3), np.int64)
        return e, e, np.zeros((0, 3), np.float32), rejected
    return np.concatenate(Xs), np.concatenate(Ys), np.concatenate(Zs), rejected


def _window(X, Y, Z, i0, j0, i1, j1, sx, sy, W):
    """Fragments of triangles whose pixel boxes start at (i0, j0): an sx x sy window each -> (linear pixel index, fp32 z)."""
    px = i0[:, None, None] + np.arange(sx)[None, None, :]
    py = j0[:, None, None] + np.arange(sy)[None, :, None]
    Px, Py = 256 * px + 128, 256 * py + 128
    x0, x1, x2 = (X[:, k][:, None, None] for k in range(3))
    y0, y1, y2 = (Y[:, k][:, None, None] for k in range(3))
    area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    s = np.where(area > 0, 1, -1)
    cov = (px <= i1[:, None, None]) & (py <= j1[:, None, None])
    for (xa, ya, xb, yb) in ((x1, y1, x2, y2), (x2, y2, x0, y0), (x0, y0, x1, y1)):
        e = s * ((xb - xa) * (Py - ya) - (yb - ya) * (Px - xa))
        a, b = -(yb - ya) * s, (xb - xa) * s                     # inward normal of the edge (y down)
        tl = (a > 0) | ((a == 0) & (b > 0))
        cov &= (e > 0) | ((e == 0) & tl)
    E1 = (x0 - x2) * (Py - y2) - (y0 - y2) * (Px - x2)
    E2 = (x1 - x0) * (Py - y0) - (y1 - y0) * (Px - x0)
    z0 = Z[:, 0].astype(np.float64)[:, None, None]
    dz1 = Z[:, 1].astype(np.float64)[:, None, None] - z0
    dz2 = Z[:, 2].astype(np.float64)[:, None, None] - z0
    inv = 1.0 / area.astype(np.float64)
    z = (z0 + (E1.astype(np.float64) * dz1 + E2.astype(np.float64) * dz2) * inv).astype(np.float32)
    keep = cov & (z >= 0) & (z <= 1)
    z = np.where(z == 0, np.float32(0), z)
    lin = np.broadcast_to(py * W + px, keep.shape)[keep]
    return lin, z[keep]


def fragments(X, Y, Z, W, H, budget=1 << 22):
    """Every kept fragment of the assembled triangles: (linear pixel index int64, z float32), unordered."""
    X, Y, Z = np.asarray(X, np.int64), np.asarray(Y, np.int64), np.asarray(Z, np.float32)
    area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    i0 = np.maximum(-((128 - X.min(1)) // 256), 0)            # first centre 256 i + 128 >= min x
    i1 = np.minimum((X.max(1) - 128) // 256, W - 1)
    j0 = np.maximum(-((128 - Y.min(1)) // 256), 0)
    j1 = np.minimum((Y.max(1) - 128) // 256, H - 1)
    live = (area != 0) & (i0 <= i1) & (j0 <= j1)
    X, Y, Z, i0, i1, j0, j1 = X[live], Y[live], Z[live], i0[live], i1[live], j0[live], j1[live]
    size = np.maximum(i1 - i0 + 1, j1 - j0 + 1)
    lins, zs = [], []
    lo = 0
    for S in (1, 2, 4, 8, 16, 32, 64, 128):
        sel = np.nonzero((size > lo) & (size <= S))[0]
        lo = S
        step = max(1, budget // (S * S))
        for c in range(0, len(sel), step):
            k = sel[c:c + step]
            l, z = _window(X[k], Y[k], Z[k], i0[k], j0[k], i1[k], j1[k], S, S, W)
            lins.append(l); zs.append(z)
    for t in np.nonzero(size > 128)[0]:                       # big boxes: one triangle at a time, in bands of rows
        sx = int(i1[t] - i0[t] + 1)
        rows = max(1, budget // sx)
        for r in range(int(j0[t]), int(j1[t]) + 1, rows):
            sy = min(rows, int(j1[t]) + 1 - r)
            k = slice(t, t + 1)
            l, z = _window(X[k], Y[k], Z[k], i0[k], np.array([r]), i1[k], np.array([r + sy - 1]), sx, sy, W)
            lins.append(l); zs.append(z)
    if not lins:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    return np.concatenate(lins), np.concatenate(zs)


def raster(depth, pos, indices, draws):
    """The pass on `depth` (float32 [H][W], not modified): returns (new map, rejected triangle count)."""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    X, Y, Z, rejected = assemble(pos, indices, draws, W, H)
    lin, z = fragments(X, Y, Z, W, H)
    out = depth.copy().ravel()
    np.minimum.at(out, lin, z)
    return out.reshape(H, W), rejected


def crowded_triangles(W, H, seed=0x5EED12C0):
    """Input of the K12 and K13 GPU tests that load the paths a small random scene never reaches: one triangle over the whole target
    (its pixel box touches every tile), 260 small ones inside the tile at (64, 64) and six across the right and bottom edges.
    Returns (tris float64 [n][3][2] in pixels, multiples of 1/8, all of negative area: counter-clockwise on a y-down screen;
    depth float64 [n], distinct, the large triangle behind everything)."""
    rng = np.random.default_rng(seed)
    big = [[(-10.0, -10.0), (-10.0, 2.0 * H + 20.0), (2.0 * W + 20.0, -10.0)]]
    c = rng.uniform(67.0, 93.0, (260, 1, 2))
    small = c + np.array([(-2.0, -2.0), (0.0, 2.0), (2.0, -1.0)]) + rng.uniform(-0.5, 0.5, (260, 3, 2))
    edge = [[(W - 10.0, 20.0), (W - 5.0, 50.0), (W + 15.0, 30.0)], [(W - 1.5, 60.0), (W - 0.25, 70.0), (W + 40.0, 64.0)],
            [(50.0, H - 8.0), (60.0, H - 0.75), (90.0, H + 12.0)], [(100.0, H - 1.5), (104.0, H + 30.0), (130.0, H - 1.25)],
            [(W - 20.0, H - 20.0), (W - 12.0, H + 9.0), (W + 9.0, H - 12.0)], [(W - 1.5, H - 1.5), (W - 1.0, H + 5.0), (W + 5.0, H - 1.0)]]
    tris = np.rint(np.concatenate([np.array(big), small, np.array(edge)]) * 8.0) / 8.0
    x, y = tris[..., 0], tris[..., 1]
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    assert (area < 0).all()
    m = len(tris)
    depth = np.concatenate([[0.9], rng.permutation(np.arange(1, m)) / (m + 2.0) * 0.8])
    return tris, depth


def tile_load(tris, W, H, tile=32, max_tiles=16):
    """What triangles given in pixels ask of the tile structure of DESIGN.md K12: (bin size of every tile [ty][tx], number of triangles
    whose pixel box touches more than `max_tiles` tiles).  Boxes by the contract's rule: the pixel centres inside the bounding box."""
    tx, ty = -(-W // tile), -(-H // tile)
    bins, large = np.zeros((ty, tx), np.int64), 0
    for t in np.asarray(tris, np.float64):
        i0, i1 = max(int(np.ceil(t[:, 0].min() - 0.5)), 0), min(int(np.floor(t[:, 0].max() - 0.5)), W - 1)
        j0, j1 = max(int(np.ceil(t[:, 1].min() - 0.5)), 0), min(int(np.floor(t[:, 1].max() - 0.5)), H - 1)
        if i0 > i1 or j0 > j1:
            continue
        a0, a1, b0, b1 = i0 // tile, i1 // tile, j0 // tile, j1 // tile
        if (a1 - a0 + 1) * (b1 - b0 + 1) > max_tiles:
            large += 1
        else:
            bins[b0:b1 + 1, a0:a1 + 1] += 1
    return bins, large
