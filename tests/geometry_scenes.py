"""Scenes of the geometry pass (K13) shared by the CPU tests, the host build of geometry_core.h and the GPU tests, and their CPU
reference (tests/geometry_raster_ref.py).  No GPU here.

A scene: dict(W, H, materials [[base, normal, orm, emissive] uint8 images], meshes [(vertices float32 [n][11], indices uint32)],
passes [dict(clear, draws [dict(m, m_old float32[16] (column-major), jitter, jitter_prev, material, mesh, vertices, indices,
index_count, first_index, vertex_offset)])]).
"""
import numpy as np

import geometry_raster_ref as G
import sun_raster_ref as R

f32 = np.float32


def perspective(W, H, eye=(0.0, 0.0, 0.0), fov=70.0, near=0.1, far=100.0):
    """Column-major float32[16]: camera at `eye` looking down -z, depth 0 (near) .. 1 (far), y down on screen as in Vulkan."""
    t = 1.0 / np.tan(np.radians(fov) / 2)
    P = np.array([[t * H / W, 0, 0, 0], [0, -t, 0, 0], [0, 0, far / (near - far), near * far / (near - far)], [0, 0, -1, 0]], np.float64)
    V = np.eye(4)
    V[:3, 3] = -np.asarray(eye, np.float64)
    return (P @ V).T.astype(f32).ravel()


def vertices(pos, uv=None, nrm=None):
    pos = np.asarray(pos, f32)
    v = np.zeros((len(pos), 11), f32)
    v[:, 0:3] = pos
    v[:, 3:6] = (0.0, 0.0, 1.0) if nrm is None else nrm
    v[:, 6:9] = (1.0, 0.0, 0.0)
    if uv is not None:
        v[:, 9:11] = uv
    return v


def flat_material(size=32, seed=1):
    """Opaque material whose emissive texels are all distinct: a triangle with one uv on a texel centre shows that texel's colour."""
    rng = np.random.default_rng(seed)
    base = np.full((size, size, 4), 255, np.uint8)
    base[..., :3] = rng.integers(0, 256, (size, size, 3))
    nrm = np.full((size, size, 4), 128, np.uint8)
    orm = rng.integers(0, 256, (size, size, 4)).astype(np.uint8)
    k = np.arange(size * size).reshape(size, size)
    emi = np.stack([k % 256, k // 256 * 16 + 7, (k * 7) % 256, np.full_like(k, 255)], -1).astype(np.uint8)
    return [base, nrm, orm, emi]


def tie_grid_scene(W=64):
    """Screen-aligned triangles sharing edges and vertices on pixel centres (orthographic pixel matrix), each with its own depth
    and its own emissive texel; drawn counter-clockwise on screen."""
    rng = np.random.default_rng(0x5EED1301)
    n = 8
    Pg = np.zeros((n + 1, n + 1, 2))
    for a in range(n + 1):
        for b in range(n + 1):
            jit = rng.integers(-2, 3, 2) if 0 < a < n and 0 < b < n else (0, 0)
            Pg[a, b] = (8 * a + jit[0], 8 * b + jit[1])
    Pg = Pg - 0.5                                                            # corners on pixel CORNERS at the rim (-0.5 .. W - 0.5 + 0.5): see below
    Pg[1:n, 1:n] += 1.0                                                      # inner vertices on pixel centres
    Pg[0, :, 0] = 0.0; Pg[n, :, 0] = W; Pg[:, 0, 1] = 0.0; Pg[:, n, 1] = W   # the rim on the target's edge: every pixel is covered
    Pg[1:n, 0, 0] += 1.0; Pg[1:n, n, 0] += 1.0; Pg[0, 1:n, 1] += 1.0; Pg[n, 1:n, 1] += 1.0
    tris = []
    for a in range(n):
        for b in range(n):
            p00, p10, p01, p11 = Pg[a, b], Pg[a + 1, b], Pg[a, b + 1], Pg[a + 1, b + 1]
            tris += [[p00, p11, p10], [p00, p01, p11]] if rng.random() < 0.5 else [[p00, p01, p10], [p10, p01, p11]]
    tris += [[rng.integers(0, W, 2) + 0.5 for _ in range(3)] for _ in range(60)]     # either winding: about half are culled
    tris = np.array(tris, np.float64)
    m = len(tris)
    depth = (rng.permutation(m) + 1).astype(np.float64) / (m + 2)
    depth[5] = depth[70]                                                             # equal depths where triangles overlap: lower index wins
    pos = np.concatenate([tris.reshape(-1, 2), np.repeat(depth, 3)[:, None]], 1)
    k = np.arange(m)
    uv = np.repeat(np.stack([(k % 32 + 0.5) / 32, (k // 32 + 0.5) / 32], 1), 3, 0)
    M = R.pixel_matrix(W, W)
    draw = dict(m=M, m_old=M, jitter=(0.0, 0.0), jitter_prev=(0.0, 0.0), material=0, vertices=vertices(pos, uv),
                indices=np.arange(3 * m, dtype=np.uint32), index_count=3 * m, first_index=0, vertex_offset=0, mesh=0)
    return dict(W=W, H=W, materials=[flat_material()], meshes=[(draw["vertices"], draw["indices"])], passes=[dict(clear=True, draws=[draw])])


def random_scene(W=64, H=48, n=300, seed=0x5EED1302):
    """Random triangles under a perspective camera: slivers, zero-area ones, near-plane crossers, ones far larger than the guard band,
    one NaN vertex and one out-of-range index; textured with alpha-tested materials; jittered, with a moved old camera."""
    from pbrhip import synth
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-6, 6, n), rng.uniform(-4, 4, n), rng.uniform(-9, -1.5, n)], 1)[:, None, :]
    size = np.exp(rng.uniform(np.log(0.05), np.log(4.0), (n, 1, 1)))
    p = c + rng.normal(size=(n, 3, 3)) * size
    q = n // 20
    p[0:q, 1] = p[0:q, 0]                                                    # zero area: repeated vertex
    p[q:2 * q, 2] = p[q:2 * q, 0] + 1e-3 * (p[q:2 * q, 1] - p[q:2 * q, 0])  # slivers
    p[2 * q:3 * q, 0, 2] = rng.uniform(0.2, 3.0, q)                          # near-plane crossers: one corner behind the camera
    p[3 * q:4 * q] *= (1.0, 1.0, 0.02)
    p[3 * q:4 * q, :, 2] -= 0.12                                             # just behind the near plane and far wider than the guard band
    p[3 * q:4 * q, :, 0:2] *= 40.0
    pos = p.reshape(-1, 3).astype(f32)
    pos[3 * (4 * q) + 1, 1] = np.nan                                         # one NaN vertex
    nrm = rng.normal(size=(3 * n, 3)).astype(f32)
    uv = rng.uniform(-2.0, 3.0, (3 * n, 2)).astype(f32)
    idx = np.arange(3 * n, dtype=np.uint32)
    idx[3 * (5 * q) + 2] = 3 * n + 17                                        # one out-of-range index
    flip = rng.random(n) < 0.5                                               # either winding: about half are counter-clockwise
    idx2 = idx.reshape(n, 3).copy()
    idx2[flip] = idx2[flip][:, [0, 2, 1]]
    idx = idx2.ravel()
    mats = synth.synth_materials(2, 32, seed=seed)
    M = perspective(W, H)
    Mo = perspective(W, H, eye=(0.05, -0.02, 0.1))
    v = vertices(pos, uv, nrm)
    h = 3 * (n // 2)
    common = dict(m=M, m_old=Mo, jitter=(0.25 / W, -0.125 / H), jitter_prev=(-0.3 / W, 0.2 / H), vertices=v, indices=idx, vertex_offset=0, mesh=0)
    draws = [dict(common, material=0, index_count=h, first_index=0), dict(common, material=1, index_count=3 * n - h, first_index=h)]
    return dict(W=W, H=H, materials=mats, meshes=[(v, idx)], passes=[dict(clear=True, draws=draws)])


def two_draw_scene(W=64, H=40):
    """A mesh and a 'skybox' with their own buffers and materials in one pass, then a second pass instance onto the first's depth."""
    a = random_scene(W, H, 120, seed=0x5EED1303)
    b = random_scene(W, H, 60, seed=0x5EED1304)
    da, db = a["passes"][0]["draws"], b["passes"][0]["draws"]
    for d in db:
        d["mesh"] = 1
        d["material"] += 2
        d["m"], d["m_old"], d["jitter"], d["jitter_prev"] = da[0]["m"], da[0]["m_old"], da[0]["jitter"], da[0]["jitter_prev"]
    c = random_scene(W, H, 80, seed=0x5EED1305)
    dc = c["passes"][0]["draws"]
    for d in dc:
        d["mesh"] = 2
    return dict(W=W, H=H, materials=a["materials"] + b["materials"], meshes=a["meshes"] + b["meshes"] + c["meshes"],
                passes=[dict(clear=True, draws=da + db), dict(clear=False, draws=dc)])


def crowded_scene(W, H):
    """R.crowded_triangles under the orthographic pixel matrix: a triangle over the whole target behind everything, 260 in one tile, six
    across the right and bottom edges; each with its own depth and its own emissive texel."""
    tris, depth = R.crowded_triangles(W, H)
    m = len(tris)
    pos = np.concatenate([tris.reshape(-1, 2), np.repeat(depth, 3)[:, None]], 1)
    k = np.arange(m)
    uv = np.repeat(np.stack([(k % 32 + 0.5) / 32, (k // 32 + 0.5) / 32], 1), 3, 0)
    M = R.pixel_matrix(W, H)
    draw = dict(m=M, m_old=M, jitter=(0.0, 0.0), jitter_prev=(0.0, 0.0), material=0, vertices=vertices(pos, uv),
                indices=np.arange(3 * m, dtype=np.uint32), index_count=3 * m, first_index=0, vertex_offset=0, mesh=0)
    return dict(W=W, H=H, tris=tris, materials=[flat_material()], meshes=[(draw["vertices"], draw["indices"])], passes=[dict(clear=True, draws=[draw])])


def reference(scene):
    """The scene on the CPU: targets after every pass, winner maps, rejected count."""
    W, H = scene["W"], scene["H"]
    chains = [[G.mip_chain(im) for im in mat] for mat in scene["materials"]]
    t = dict(base=np.zeros((H, W, 4), np.uint8), nrm=np.zeros((H, W, 4), np.uint8), orm=np.zeros((H, W, 4), np.uint8),
             emi=np.zeros((H, W, 4), np.uint8), vel=np.zeros((H, W, 2), np.float16), depth=np.zeros((H, W), f32))
    wins, rejected = [], 0
    for ps in scene["passes"]:
        if ps["clear"]:
            t["depth"] = np.ones((H, W), f32)
        t, win, rej = G.raster(t, [dict(d, material=chains[d["material"]]) for d in ps["draws"]])
        wins.append(win)
        rejected += rej
    return t, wins, rejected


_REF = {}


def ref_of(key, builder):
    if key not in _REF:
        scene = builder()
        _REF[key] = (scene,) + reference(scene)
    return _REF[key]
