"""The CPU reference of the sun depth pass (tests/sun_raster_ref.py) against answers derived by hand from the K12 contract
(DESIGN.md): pixel sets, the top-left tie rule, depth arithmetic, the depth range, the w divide, -0 and the rejection counts."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sun_raster_ref as R  # noqa: E402


def frags(tris, W=8, H=8, z=None, M=None):
    """tris: [[(x, y), (x, y), (x, y)], ...] in framebuffer pixels -> per-pixel coverage count and the fragments."""
    tris = np.asarray(tris, np.float32)
    n = len(tris)
    zz = np.full((n, 3), 0.5, np.float32) if z is None else np.asarray(z, np.float32).reshape(n, 3)
    pos = np.concatenate([tris.reshape(-1, 2), zz.reshape(-1, 1)], 1)
    M = R.pixel_matrix(W, H) if M is None else M
    X, Y, Z, rej = R.assemble(pos, np.arange(3 * n, dtype=np.uint32), [(3 * n, 1, 0, 0, M)], W, H)
    lin, zf = R.fragments(X, Y, Z, W, H)
    return np.bincount(lin, minlength=W * H).reshape(H, W), lin, zf, rej


def test_pixel_matrix_maps_pixels_exactly():
    xs = np.array([[0.5, 3.25, 0.0], [7.5, 0.5, 1.0], [4.0, 4.0, 0.25]], np.float32)
    xf, yf, zd = R.transform(xs, R.pixel_matrix(8, 8), 8, 8)
    assert np.array_equal(xf, xs[:, 0]) and np.array_equal(yf, xs[:, 1]) and np.array_equal(zd, xs[:, 2])


def test_small_triangle_exact_pixel_set():
    # vertices on the centres (0,0), (4,0), (0,4): the top and left edges are in, the hypotenuse (i + j == 4) is out
    cnt, _, _, _ = frags([[(0.5, 0.5), (4.5, 0.5), (0.5, 4.5)]])
    want = np.zeros((8, 8), int)
    for j in range(8):
        for i in range(8):
            want[j, i] = i + j <= 3
    assert np.array_equal(cnt, want)
    # the same triangle wound the other way covers the same centres (two-sided)
    cnt2, _, _, _ = frags([[(0.5, 0.5), (0.5, 4.5), (4.5, 0.5)]])
    assert np.array_equal(cnt2, want)
    # a triangle strictly between centres: (1.2,1.2) (2.8,1.2) (1.2,2.8) holds only the centre (1.5, 1.5)
    cnt3, _, _, _ = frags([[(1.2, 1.2), (2.8, 1.2), (1.2, 2.8)]])
    assert cnt3.sum() == 1 and cnt3[1, 1] == 1


def test_tie_rule_on_edges_and_vertices():
    # right edge x = 2.5 (vertical, inside to the left) excludes the centres on it; left edge x = 0.5 includes them
    cnt, _, _, _ = frags([[(0.5, 0.5), (2.5, 0.5), (2.5, 4.5)], [(0.5, 0.5), (2.5, 4.5), (0.5, 4.5)]])
    want = np.zeros((8, 8), int)
    want[0:4, 0:2] = 1                                       # columns 0, 1 and rows 0..3: the bottom edge y = 4.5 is out
    assert np.array_equal(cnt, want)
    # a centre exactly on a shared vertex belongs to one triangle only (here the fan below)


def test_grid_and_fan_cover_every_centre_once():
    # 4 x 4 squares of 1.5 px split along alternating diagonals, vertices on 1/4-pixel positions and on centres
    tris = []
    for a in range(4):
        for b in range(4):
            x0, y0, x1, y1 = 0.5 + 1.5 * a, 0.5 + 1.5 * b, 0.5 + 1.5 * (a + 1), 0.5 + 1.5 * (b + 1)
            if (a + b) % 2:
                tris += [[(x0, y0), (x1, y0), (x1, y1)], [(x0, y0), (x1, y1), (x0, y1)]]
            else:
                tris += [[(x0, y0), (x1, y0), (x0, y1)], [(x1, y0), (x1, y1), (x0, y1)]]
    cnt, _, _, _ = frags(tris)
    want = np.zeros((8, 8), int)
    want[0:6, 0:6] = 1                                       # centres 0.5 .. 5.5 inside [0.5, 6.5): the right / bottom border is out
    assert np.array_equal(cnt, want)
    # a fan of 12 triangles around the centre (4.5, 4.5) with rim vertices on centres of a 7 x 7 square
    rim = [(1.5, 1.5), (4.5, 1.5), (7.5, 1.5), (7.5, 4.5), (7.5, 7.5), (4.5, 7.5), (1.5, 7.5), (1.5, 4.5)]
    rim = rim + [rim[0]]
    fan = [[(4.5, 4.5), rim[k], rim[k + 1]] for k in range(8)]
    cnt, _, _, _ = frags(fan, W=10, H=10)
    want = np.zeros((10, 10), int)
    want[1:7, 1:7] = 1                                       # the square [1.5, 7.5]^2: top and left borders in, the others out
    assert np.array_equal(cnt, want)


def test_constant_depth_and_planar_ramp():
    _, _, z, _ = frags([[(0.5, 0.5), (6.5, 0.5), (0.5, 6.5)]], z=[0.3] * 3)
    assert len(z) and np.all(z == np.float32(0.3))
    # z = (x - 0.5) / 8 on a right triangle with 8-px legs: every centre value is binary-exact and must come out exact
    _, lin, z, _ = frags([[(0.5, 0.5), (8.5, 0.5), (0.5, 8.5)]], W=16, H=16, z=[0.0, 1.0, 0.0])
    x = lin % 16
    assert len(z) == 36 and np.array_equal(z, ((x + 0.5 - 0.5) / 8).astype(np.float32))


def test_depth_range_is_inclusive():
    one_up = np.nextafter(np.float32(1), np.float32(2))
    for zc, kept in ((0.0, True), (1.0, True), (float(one_up), False), (-1e-30, False), (-0.0, True)):
        _, _, z, _ = frags([[(0.5, 0.5), (4.5, 0.5), (0.5, 4.5)]], z=[zc] * 3)
        assert (len(z) > 0) == kept, zc
    # -0.0 is written as +0.0
    _, _, z, _ = frags([[(0.5, 0.5), (4.5, 0.5), (0.5, 4.5)]], z=[-0.0] * 3)
    assert np.all(z.view(np.uint32) == 0)
    # a ramp through the range keeps exactly the fragments with 0 <= z <= 1
    _, lin, z, _ = frags([[(0.5, 0.5), (8.5, 0.5), (0.5, 8.5)]], W=16, H=16, z=[-0.5, 1.5, -0.5])
    assert len(z) and z.min() >= 0 and z.max() <= 1 and len(z) < 36


def test_w_is_divided():
    # the pose-2 matrix has w = 1.0000001: xd = cx / w exactly, no shortcut through w == 1
    M = R.pixel_matrix(8, 8)
    M2 = M.copy()
    M2[15] = np.float32(1.0000001)
    p = np.array([[3.3, 2.2, 0.7]], np.float32)
    xf, yf, zd = R.transform(p, M2, 8, 8)
    m = M2
    cx = ((m[0] * p[0, 0] + m[4] * p[0, 1]) + m[8] * p[0, 2]) + m[12]
    want = np.float32(4) * (cx / m[15]) + np.float32(4)
    assert xf[0] == want and zd[0] == p[0, 2] / m[15] and zd[0] != p[0, 2]
    # w = 2 with the other rows doubled gives the same result as w = 1
    a, _, za, _ = frags([[(0.5, 0.5), (4.5, 0.5), (0.5, 4.5)]], M=R.pixel_matrix(8, 8, w=2.0))
    b, _, zb, _ = frags([[(0.5, 0.5), (4.5, 0.5), (0.5, 4.5)]])
    assert np.array_equal(a, b) and np.array_equal(za, zb)


def test_min_with_target_and_rejection_counts():
    W = H = 8
    pos = np.array([[0.5, 0.5, 0.25], [4.5, 0.5, 0.25], [0.5, 4.5, 0.25],            # 0..2 drawn
                    [0.5, 0.5, 0.75], [6.5, 0.5, 0.75], [0.5, 6.5, 0.75],            # 3..5 behind it where they overlap
                    [2.0 ** 21 + 1, 0.5, 0.5], [np.nan, 0.5, 0.5], [1.0, 1.0, np.inf],  # 6 guard band, 7 NaN, 8 inf depth
                    [2.0, 2.0, 0.1], [2.0, 2.0, 0.1]], np.float32)                   # 9, 10: degenerate
    idx = np.array([0, 1, 2, 3, 4, 5, 6, 0, 1, 7, 1, 2, 8, 0, 1, 9, 10, 9, 0, 1, 99], np.uint32)
    M = R.pixel_matrix(W, H)
    init = np.full((H, W), 1.0, np.float32)
    init[7, 7] = 0.125
    out, rej = R.raster(init, pos, idx, [(21, 1, 0, 0, M)])
    assert rej == 4                                           # guard band, NaN, inf, index 99 past the 11 vertices
    assert out[7, 7] == np.float32(0.125)                     # an earlier value smaller than every fragment stays
    assert out[0, 0] == np.float32(0.25) and out[0, 5] == np.float32(0.75) and out[6, 6] == 1.0
    # instance_count 0 draws nothing; any larger count draws once; index_count rounds down to whole triangles
    o0, _ = R.raster(init, pos, idx, [(3, 0, 0, 0, M)])
    assert np.array_equal(o0, init)
    o1, _ = R.raster(init, pos, idx, [(5, 7, 0, 0, M)])
    o2, _ = R.raster(init, pos, idx, [(3, 1, 0, 0, M)])
    assert np.array_equal(o1, o2)
    # vertex_offset and first_index select the second triangle
    o3, _ = R.raster(init, pos, np.array([0, 1, 2], np.uint32), [(3, 1, 0, 3, M)])
    o4, _ = R.raster(init, pos, idx, [(3, 1, 3, 0, M)])
    assert np.array_equal(o3, o4) and o3[0, 5] == np.float32(0.75)
