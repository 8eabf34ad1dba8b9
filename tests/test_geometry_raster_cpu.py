"""Pins the CPU reference of the geometry pass contract (tests/geometry_raster_ref.py) by hand-derived cases.
No GPU, no library: what touches the library (mip generation through GPU_MakeTexture) is checked in tests/test_gpu_geometry.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_raster_ref as G  # noqa: E402
import sun_raster_ref as R  # noqa: E402
from geometry_scenes import perspective  # noqa: E402

f32 = np.float32
T_FOV = 1.0 / np.tan(np.radians(70.0) / 2)                   # perspective()'s focal scale at its default field of view


def _const_material(rgba_base=(255, 255, 255, 255), size=4):
    img = lambda c: np.tile(np.array(c, np.uint8), (size, size, 1))  # noqa: E731
    return [G.mip_chain(img(rgba_base)), G.mip_chain(img((128, 128, 255, 255))), G.mip_chain(img((255, 128, 64, 255))), G.mip_chain(img((10, 20, 30, 255)))]


def _draw(M, pos, material, uv=None, Mo=None, jitter=(0.0, 0.0), jitter_prev=(0.0, 0.0)):
    pos = np.asarray(pos, f32)
    v = np.zeros((len(pos), 11), f32)
    v[:, 0:3] = pos
    v[:, 3:6] = (0.0, 0.0, 1.0)
    if uv is not None:
        v[:, 9:11] = uv
    return dict(m=M, m_old=M if Mo is None else Mo, jitter=jitter, jitter_prev=jitter_prev, material=material, vertices=v,
                indices=np.arange(len(v), dtype=np.uint32), index_count=len(v), first_index=0, vertex_offset=0)


def _targets(W, H):
    return dict(base=np.zeros((H, W, 4), np.uint8), nrm=np.zeros((H, W, 4), np.uint8), orm=np.zeros((H, W, 4), np.uint8),
                emi=np.zeros((H, W, 4), np.uint8), vel=np.zeros((H, W, 2), np.float16), depth=np.ones((H, W), f32))


TRI = [(0.5, 0.5, 0.25), (0.5, 6.5, 0.5), (6.5, 0.5, 0.75)]          # counter-clockwise on the screen (y down): area -36 px^2


def test_hand_computed_triangle_8x8():
    """Orthographic pixel matrix (w = 1): lambda_B = j / 6, lambda_C = i / 6, depth = 0.25 + 0.25 j / 6 + 0.5 i / 6; the corner pixel
    (0, 0) sits on a left and a top edge (covered), the hypotenuse i + j = 6 is a right/bottom edge (not covered)."""
    M = R.pixel_matrix(8, 8)
    d = _draw(M, TRI, _const_material(), uv=[(p[0] / 8, p[1] / 8) for p in TRI])
    out, win, rej = G.raster(_targets(8, 8), [d])
    assert rej == 0
    want = np.array([[i + j < 6 and i <= 5 and j <= 5 for i in range(8)] for j in range(8)])
    assert np.array_equal(win >= 0, want)
    A, fans = G.setup(d, d["vertices"], 8, 8)
    assert fans == [((128, 128), (128, 1664), (1664, 128))]
    for i, j in ((0, 0), (2, 1), (1, 3)):
        lam = G.lambdas(A, np.array([i]), np.array([j]), 8, 8)
        for got, expect in zip(lam, (1 - (i + j) / 6, j / 6, i / 6)):
            assert abs(got[0] - expect) < 1e-12
        z = 0.25 + 0.25 * j / 6 + 0.5 * i / 6
        assert abs(float(out["depth"][j, i]) - z) <= 2.0 ** -24
    assert out["depth"][0, 0] == f32(0.25) and out["depth"][3, 3] == 1.0
    assert tuple(out["emi"][1, 1]) == (10, 20, 30, 255) and tuple(out["orm"][1, 1]) == (255, 128, 64, 255)
    # uv = xy / 8: T = (1, 0, 0), B = cross(T, N) = (0, -1, 0); the texel (128, 128) / 255 is +0.0039 in x and y of tangent space
    assert tuple(out["nrm"][1, 1]) == (128, 127, 255, 255)
    assert tuple(out["emi"][7, 7]) == (0, 0, 0, 0)                        # nobody won: previous contents


def test_culling_draws_counter_clockwise_only():
    """gpu_vulkan.c maps GPU_CullMode_DrawCCW to cullMode BACK with the default front face (counter-clockwise): the triangle whose
    framebuffer-space area (y down) is negative is drawn, its mirror image is not."""
    M = R.pixel_matrix(8, 8)
    ccw, _, _ = G.raster(_targets(8, 8), [_draw(M, TRI, _const_material())])
    cw, win, _ = G.raster(_targets(8, 8), [_draw(M, [TRI[0], TRI[2], TRI[1]], _const_material())])
    assert (ccw["depth"] < 1).sum() == 21 and (cw["depth"] < 1).sum() == 0 and (win == -1).all()


def test_depth_tie_lower_index_wins_and_discard_reveals():
    M = R.pixel_matrix(8, 8)
    flat = [(p[0], p[1], 0.5) for p in TRI]
    two = _draw(M, flat + flat, _const_material())
    out, win, _ = G.raster(_targets(8, 8), [two])
    assert set(np.unique(win)) == {-1, 0}                                 # equal depth: LESS keeps the first
    near = [(p[0], p[1], 0.25) for p in TRI]
    holes = _draw(M, near, _const_material((255, 255, 255, 76)))          # alpha 76 / 255 = 0.298 < 0.3: every fragment is discarded
    solid = _draw(M, flat, _const_material((255, 255, 255, 77)))          # 77 / 255 = 0.302: kept
    out, win, _ = G.raster(_targets(8, 8), [holes, solid])
    assert set(np.unique(win)) == {-1, 1} and (out["depth"][win == 1] == f32(0.5)).all()


def test_near_plane_split_floor():
    """A floor triangle (y = -1) from far in front of the camera to behind it, wider than the guard band: with y_n = t / s for the
    floor point at distance s, exactly the pixel rows with t / far < y_n are covered, at depth (far / (near - far)) (1 - near / s) ... """
    W = H = 16
    M, t = perspective(W, H), T_FOV
    near, far = 0.1, 100.0
    pos = [(-4000.0, -1.0, -3000.0), (0.0, -1.0, 500.0), (4000.0, -1.0, -3000.0)]
    outs = []
    for order in ((0, 1, 2), (0, 2, 1)):
        out, win, rej = G.raster(_targets(W, H), [_draw(M, [pos[k] for k in order], _const_material())])
        assert rej == 0
        outs.append((out, win))
    drawn = [o for o in outs if (o[1] >= 0).any()]
    assert len(drawn) == 1                                                # one winding is culled, whole
    out, win = drawn[0]
    yn = (2 * np.arange(H) + 1) / H - 1
    assert np.array_equal(win >= 0, np.repeat((yn > t / far)[:, None], W, 1))
    for j in range(8, 16):
        s = t / yn[j]
        z = (far / (near - far) * -s + near * far / (near - far)) / s
        assert np.abs(out["depth"][j].astype(np.float64) - z).max() < 2e-6


def test_lod_levels_and_blend():
    """A footprint of r texels per pixel gives level log2 r: 0, 1 and 2 exactly at r = 1, 2, 4; r = 3 blends levels 1 and 2."""
    tex = [np.full((32 >> l, 32 >> l, 4), 40 * l, np.uint8) for l in range(6)]
    for r, want in ((1.0, 0.0), (2.0, 1.0), (4.0, 2.0), (0.3, 0.0), (1e9, 5.0)):
        lod, bad = G.lod_of(tex, np.array([[r / 32, 0.0]], f32), np.array([[0.0, r / 32]], f32))
        assert lod[0] == f32(want) and not bad[0], (r, lod)
    lod, _ = G.lod_of(tex, np.array([[3 / 32, 0.0]], f32), np.array([[0.0, 1 / 32]], f32))
    assert abs(float(lod[0]) - np.log2(3.0)) <= 2.0 ** -9 + 2.0 ** -9    # polynomial bound + snap to 1/256
    uv = np.array([[0.37, 0.81]], f32)
    c = G.texture(tex, uv, np.array([[3 / 32, 0.0]], f32), np.array([[0.0, 1 / 32]], f32))
    frac = lod[0] - f32(1)
    c1, c2 = f32(40) / f32(255), f32(80) / f32(255)
    assert c[0, 0] == c1 + frac * (c2 - c1)
    # non-finite footprint or coordinate: coarsest level
    c = G.texture(tex, np.array([[np.nan, 0.5]], f32), np.zeros((1, 2), f32), np.zeros((1, 2), f32))
    assert c[0, 0] == f32(200) / f32(255)
    c = G.texture(tex, uv, np.array([[np.inf, 0.0]], f32), np.zeros((1, 2), f32))
    assert c[0, 0] == f32(200) / f32(255)


def test_bilinear_repeat_and_snap():
    lvl = np.zeros((2, 2, 4), np.uint8)
    lvl[0, 0], lvl[0, 1], lvl[1, 0], lvl[1, 1] = 0, 255, 51, 102
    at = lambda u, v: G.bilinear(lvl, np.array([u], f32), np.array([v], f32))[0, 0]  # noqa: E731
    assert at(0.25, 0.25) == 0 and at(0.75, 0.25) == 1 and at(1.25, -0.75) == 0      # texel centres, repeated
    assert at(0.5, 0.25) == f32(0.5) and at(0.0, 0.25) == f32(0.5)                   # halfway, and across the wrap
    assert at(0.25 + 1.0 / 2048, 0.25) == 0                                          # 1/1024 texel: snapped away (1/256 grid)


def test_mip_chain_by_hand():
    a = np.zeros((4, 4, 4), np.uint8)
    a[0:2, 0:2, 0] = [[0, 0], [255, 255]]          # 0.5 -> rint(127.5) = 128 (ties to even)
    a[0:2, 2:4, 0] = [[10, 20], [30, 40]]          # 25
    a[2:4, 0:2, 0] = [[0, 0], [0, 1]]              # 0.25 -> 0
    a[2:4, 2:4, 0] = [[3, 3], [3, 4]]              # 3.25 -> 3
    chain = G.mip_chain(a)
    assert [l.shape[0] for l in chain] == [4, 2, 1]
    assert chain[1][..., 0].tolist() == [[128, 25], [0, 3]]
    assert chain[2][0, 0, 0] == 39                 # (128 + 25 + 0 + 3) / 4 = 39


def test_log2_polynomial_bound():
    m = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3F800000)).view(f32)
    err = np.abs(G.log2_poly(m).astype(np.float64) - np.log2(m.astype(np.float64))).max()
    print(f"log2 polynomial: worst error {err:.3g} level over all 2^23 mantissas / bound 2^-9 = {2.0 ** -9:.3g}")
    assert err <= 2.0 ** -9
    for k in (1, 7, 13):
        x = (m[::4097] * f32(2.0 ** k)).astype(f32)
        assert np.abs(G.log2_poly(x).astype(np.float64) - np.log2(x.astype(np.float64))).max() <= 2.0 ** -9
    assert G.log2_poly(f32(2.0)) == 1 and G.log2_poly(f32(4.0)) == 2 and G.log2_poly(f32(1024.0)) == 10


def test_velocity_of_a_camera_translation():
    """Static wall at z = -5, old camera moved by (dx, dy, 0): velocity = (t (H/W) dx / 5, -t dy / 5) everywhere, jitter cancelled."""
    W, H = 16, 8
    dx, dy = 0.3, -0.2
    M, t = perspective(W, H), T_FOV
    Mo = perspective(W, H, eye=(dx, dy, 0.0))
    wall = [(-40.0, 30.0, -5.0), (-40.0, -30.0, -5.0), (40.0, 30.0, -5.0)]
    outs = [G.raster(_targets(W, H), [_draw(M, [wall[k] for k in o], _const_material(), Mo=Mo, jitter=(0.01, -0.02), jitter_prev=(-0.03, 0.015))])
            for o in ((0, 1, 2), (0, 2, 1))]
    out, win, _ = [o for o in outs if (o[1] >= 0).any()][0]
    assert (win >= 0).mean() > 0.4
    want = np.array([t * (H / W) * dx / 5, -t * dy / 5])
    got = out["vel"][win >= 0].astype(np.float64)
    assert np.abs(got - want).max() <= np.abs(want).max() * 2.0 ** -11 + 1e-5


def test_rasterised_quad_lod_1_2_4_and_between():
    """A screen-aligned 16 x 16 quad (two triangles, orthographic pixel matrix) over a 16^2 texture whose level l is the constant 40 l:
    r texels per pixel in x (and fewer in y) select level log2 r through pix() -- odd minus even in both directions -- and texture()."""
    W = 16
    M = R.pixel_matrix(W, W)
    chain = [np.full((16 >> l, 16 >> l, 4), 40 * l, np.uint8) for l in range(5)]
    opaque = G.mip_chain(np.full((4, 4, 4), 255, np.uint8))
    corners = [(0.0, 0.0), (0.0, 16.0), (16.0, 16.0), (16.0, 0.0)]
    for r, want in ((1.0, 0), (2.0, 40), (4.0, 80)):
        for sx, sy in ((1, 1), (-1, 1), (1, -1)):                            # mirrored mappings: the footprint, not its sign, sets the level
            pos = [(x, y, 0.5) for x, y in corners]
            uv = [(sx * r * x / 16, sy * 0.5 * r * y / 16) for x, y in corners]
            quad = [0, 1, 2, 0, 2, 3]
            d = _draw(M, [pos[k] for k in quad], [opaque, chain, chain, chain], uv=[uv[k] for k in quad])
            out, win, _ = G.raster(_targets(W, W), [d])
            assert (win >= 0).all()
            assert (out["emi"][..., 0] == want).all() and (out["orm"][..., 0] == want).all(), (r, sx, sy)
    pos = [(x, y, 0.5) for x, y in corners]
    uv = [(3.0 * x / 16, y / 16) for x, y in corners]
    d = _draw(M, [pos[k] for k in quad], [opaque, chain, chain, chain], uv=[uv[k] for k in quad])
    out, _, _ = G.raster(_targets(W, W), [d])
    lod, _ = G.lod_of(chain, np.array([[3 / 16, 0.0]], f32), np.array([[0.0, 1 / 16]], f32))
    blend = f32(40) / f32(255) + (lod[0] - f32(1)) * (f32(80) / f32(255) - f32(40) / f32(255))
    assert 1.5 < lod[0] < 1.7 and (out["emi"][..., 0] == np.rint(f32(255) * blend)).all()
