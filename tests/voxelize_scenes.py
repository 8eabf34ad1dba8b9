"""Scenes of the voxelise pass (K14) shared by the CPU tests, the host build of voxelize_core.h and the GPU tests.  No GPU here.

A scene: dict(N, sun_map float32 [h][w], sun float32[16] (column-major), sun_dir (4 floats), scale, materials [[base, normal, orm,
emissive] uint8 images], meshes [(vertices float32 [n][11], indices uint32)], prior (float16 [N][N][N][4] or None = zeros),
passes [dict(clear, draws [dict(mesh, material, first_vertex, vertex_count, instance_count)])]).
World units are voxels (scale = 2 / N): world coordinate c lies at pixel / voxel c + N / 2.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_raster_ref as G  # noqa: E402
import voxelize_raster_ref as V  # noqa: E402
from geometry_scenes import flat_material, vertices  # noqa: E402

f32 = np.float32


def constant_material(base, emissive, size=4):
    im = lambda c: np.tile(np.array(list(c) + [255], np.uint8), (size, size, 1))  # noqa: E731
    return [im(base), im((128, 128, 255)), im((255, 128, 0)), im(emissive)]


def sun_setup(N, size=64, lit=False):
    """A sun looking down a tilted axis over the grid's volume and its depth map with a step, a ramp and noise: shadow 0, 1 and
    fractions all occur.  lit: a map of ones (nothing is in shadow)."""
    s = 2.0 / N
    M = np.array([[0.55 * s, 0.2 * s, 0.05 * s, 0.01], [-0.2 * s, 0.55 * s, 0.1 * s, -0.02], [0.03 * s, -0.06 * s, 0.3 * s, 0.5], [0, 0, 0, 1]], np.float64)
    sun = M.T.astype(f32).ravel()
    if lit:
        return sun, np.ones((size, size), f32)
    rng = np.random.default_rng(0x5EED1401)
    y, x = np.mgrid[0:size, 0:size]
    depth = np.where(x < size // 2, 0.35, 0.62) + 0.1 * (y / size) + rng.uniform(-0.05, 0.05, (size, size))
    return sun, depth.astype(f32)


def make_scene(N, tris, uv=None, materials=None, material_of=None, sun_dir=(-0.4, 0.5, -0.768), lit=False, prior=None, split=None):
    """tris: float [n][3][3] world positions -> a scene with one mesh, non-indexed order; split: triangle counts of the draws."""
    tris = np.asarray(tris, np.float64)
    n = len(tris)
    v = vertices(tris.reshape(-1, 3), uv)
    ix = np.arange(3 * n, dtype=np.uint32)
    sun, sun_map = sun_setup(N, lit=lit)
    split = [n] if split is None else split
    draws, first = [], 0
    for k, c in enumerate(split):
        draws.append(dict(mesh=0, material=(material_of[k] if material_of else 0), first_vertex=3 * first, vertex_count=3 * c, instance_count=1))
        first += c
    return dict(N=N, sun_map=sun_map, sun=sun, sun_dir=np.array(list(sun_dir) + [0.0], f32), scale=f32(2.0 / N),
                materials=materials or [flat_material()], meshes=[(v, ix)], prior=prior, passes=[dict(clear=prior is None, draws=draws)])


# ---- the hand-derived cases (tests/test_voxelize_raster_cpu.py writes their voxel sets out at k = 1, N = 8) ----
# coordinates are multiples of 1/64: they and their products with scale snap exactly
def case_corner(k=1):                      # z-plane, vertex A on the pixel corner (5, 5) k
    return k * np.array([[(1, 1, 0.5), (2.5, 1.25, 0.5), (1.25, 2.5, 0.5)]])


def case_edge_on_boundary(k=1):            # two edges on the pixel boundaries x = 2 k and y = 2 k
    return k * np.array([[(-2, -2, -1.5), (0, -2, -1.5), (-2, 0, -1.5)]])


def case_sliver(k=1):                      # 1/64 of a pixel thick, crosses a whole row
    return k * np.array([[(-3.5, 0.25, 2.5), (3.375, 0.5, 2.5), (3.375, 0.515625, 2.5)]])


def case_axes(k=1):                        # X-dominant, Y-dominant, and the tie |n.x| == |n.y| that goes to X
    return k * np.array([[(1.5, 0.25, 0.25), (1.5, 1.75, 0.25), (1.5, 0.25, 1.75)],
                         [(0.25, -2.5, 0.25), (0.25, -2.5, 1.75), (1.75, -2.5, 0.25)],
                         [(0.75, 0.25, 0.25), (-0.25, 1.25, 0.25), (0.75, 0.25, 1.25)]])


def case_depth_range(k=1, N=8):            # uvw N = -0.5 (voxel 0 by truncation), = N - 0.5 (voxel N - 1), = N exactly (rejected)
    t = np.array([(-3.75, -3.75, 0.0), (-2.25, -3.75, 0.0), (-3.75, -2.25, 0.0)])
    out = []
    for z in (-N / 2 - 0.5, N / 2 - 0.5, N / 2):
        q = k * t.copy()
        q[:, 2] = z
        out.append(q)
    return np.array(out)


def cases_scene(N):
    """Every hand case in one mesh, scaled by N / 8, drawn in two draws with two materials; the last draw repeats the first triangle
    (coincident: the later one wins), one triangle has zero area, one a NaN, one an index past the vertices, and the last three
    vertices' uv reads fall past the end of SSBO0."""
    k = N // 8
    tris = np.concatenate([case_corner(k), case_edge_on_boundary(k), case_sliver(k), case_axes(k), case_depth_range(k, N)])
    zero = tris[0:1].copy(); zero[0, 1] = zero[0, 0]
    nan = tris[1:2].copy(); nan[0, 2, 1] = np.nan
    tris = np.concatenate([tris, zero, nan, tris[3:4] + (0, 0, 2.0 * k), tris[0:1]])
    n = len(tris)
    rng = np.random.default_rng(0x5EED1402)
    uv = rng.uniform(-2.0, 3.0, (3 * n, 2))
    sc = make_scene(N, tris, uv, materials=[flat_material(seed=2), flat_material(seed=3)], material_of=[0, 1], split=[n - 1, 1])
    v, ix = sc["meshes"][0]
    ix = np.concatenate([ix, ix[-3:]])                                        # the last draw reads its indices from the tail ...
    ix[3 * (n - 2) + 1] = 3 * n + 5                                           # ... and the triangle before it has an index past SSBO0
    sc["meshes"][0] = (v, ix)
    sc["passes"][0]["draws"][1]["first_vertex"] = 3 * n                       # uv of vertices 3 n .. 3 n + 2: past the end, read as 0
    sc["expect"] = dict(rejected=2, last=n - 1)
    return sc


def random_scene(N=128, n=300, seed=0x5EED1403):
    """Random triangles, log-uniform 0.3 .. 60 voxels, in two draws with two materials: slivers, zero-area ones, one NaN, one bad
    index, uv in -2 .. 3, some across each face of the grid and some wholly outside, twenty exact duplicates later in the order."""
    from pbrhip import synth
    rng = np.random.default_rng(seed)
    h = N / 2.0
    c = rng.uniform(-h + 2, h - 2, (n, 1, 3))
    size = np.exp(rng.uniform(np.log(0.3), np.log(60.0), (n, 1, 1)))
    p = c + rng.normal(size=(n, 3, 3)) * size * 0.5
    q = n // 20
    p[0:q, 1] = p[0:q, 0]                                                    # zero area: repeated vertex
    p[q:2 * q, 2] = p[q:2 * q, 0] + 1e-3 * (p[q:2 * q, 1] - p[q:2 * q, 0])  # slivers
    for a in range(3):                                                       # across each face, both sides
        for s in (-1, 1):
            k = 2 * q + 2 * (2 * a + (s > 0))
            p[k:k + 2, :, a] = s * h + rng.uniform(-1.5, 1.5, (2, 3))
    p[3 * q:3 * q + 6] += (3.0 * N, 0, 0)                                    # wholly outside
    p[3 * q + 6:3 * q + 8, :, 2] = rng.uniform(-h - 0.9, -h - 0.1, (2, 3))   # just below the grid: voxel 0 by truncation
    dup = rng.choice(np.arange(4 * q, n - 40), 20, replace=False)
    p[n - 20:] = p[dup]                                                      # exact duplicates, later in the order
    pos = p.reshape(-1, 3).astype(f32)
    pos[3 * (4 * q) + 1, 1] = np.nan
    uv = rng.uniform(-2.0, 3.0, (3 * n, 2)).astype(f32)
    ix = np.arange(3 * n, dtype=np.uint32)
    ix[3 * (5 * q) + 2] = 3 * n + 17
    mats = synth.synth_materials(2, 32, seed=seed)
    for k, m in enumerate(mats):
        m[3] = flat_material(seed=10 + k)[3]                                 # distinct emissive texels
    sun, sun_map = sun_setup(N)
    half = 3 * (n // 2)
    draws = [dict(mesh=0, material=0, first_vertex=0, vertex_count=half, instance_count=1),
             dict(mesh=0, material=1, first_vertex=half, vertex_count=3 * n - half, instance_count=2)]
    return dict(N=N, sun_map=sun_map, sun=sun, sun_dir=np.array([-0.4, 0.5, -0.768, 0.0], f32), scale=f32(2.0 / N), materials=mats,
                meshes=[(vertices(pos, uv), ix)], prior=None, passes=[dict(clear=True, draws=draws)], dup=(dup, np.arange(n - 20, n)))


def load_scene(N=64):
    """One triangle per axis over the whole grid (boxes far above the small-box bound), 600 triangles inside one voxel column (heavy
    contention on a few keys), and a vertex count that is no multiple of 64, nor of 3."""
    rng = np.random.default_rng(0x5EED1404)
    h = N / 2.0
    big = np.array([[(-h - 1, -h - 1, 3.3), (h + 40, -h - 1, 3.3), (-h - 1, h + 40, 3.3)],
                    [(-7.7, -h - 1, -h - 1), (-7.7, h + 40, -h - 1), (-7.7, -h - 1, h + 40)],
                    [(-h - 1, 5.4, -h - 1), (-h - 1, 5.4, h + 40), (h + 40, 5.4, -h - 1)]])
    col = np.array([2.5, -6.5, 0.0]) + np.concatenate([rng.uniform(-0.45, 0.45, (600, 3, 2)), rng.uniform(-3.0, 3.0, (600, 3, 1))], 2)
    tris = np.concatenate([big, col])
    uv = rng.uniform(0.0, 1.0, (3 * len(tris), 2))
    sc = make_scene(N, tris, uv, split=[len(tris)])
    sc["passes"][0]["draws"][0]["vertex_count"] = 3 * len(tris) - 1          # rounded down to whole triangles
    sc["column"] = (int(2.5 + h), int(-6.5 + h))
    return sc


def two_pass_scene(N=32):
    """A pass with a clear, then a second pass instance onto the first's grid without one."""
    a, b = random_scene(N, 100, seed=0x5EED1405), random_scene(N, 80, seed=0x5EED1406)
    for d in b["passes"][0]["draws"]:
        d["mesh"] = 1
    a["meshes"] += b["meshes"]
    a["passes"].append(dict(clear=False, draws=b["passes"][0]["draws"]))
    return a


def chains(scene):
    return [[G.mip_chain(m[0]), G.mip_chain(m[3])] for m in scene["materials"]]


def ref_draws(scene, ps, ch=None):
    ch = ch or chains(scene)
    out = []
    for d in ps["draws"]:
        v, ix = scene["meshes"][d["mesh"]]
        out.append(dict(vertices=np.ascontiguousarray(v, f32).ravel(), indices=ix, vertex_count=d["vertex_count"], instance_count=d["instance_count"],
                        first_vertex=d["first_vertex"], scale=scene["scale"], sun=scene["sun"], sun_dir=scene["sun_dir"], material=ch[d["material"]]))
    return out


def reference(scene):
    """The scene on the CPU: (grids after every pass (float16), infos, rejected in all)."""
    N = scene["N"]
    ch = chains(scene)
    grid = np.zeros((N, N, N, 4), np.float16) if scene["prior"] is None else np.asarray(scene["prior"], np.float16)
    grids, infos, rejected = [], [], 0
    for ps in scene["passes"]:
        if ps["clear"]:
            grid = np.zeros((N, N, N, 4), np.float16)
        grid, info = V.voxelize(grid, scene["sun_map"], ref_draws(scene, ps, ch), N)
        grids.append(grid); infos.append(info)
        rejected += info["rejected"]
    return grids, infos, rejected


_REF = {}


def ref_of(key, builder):
    """A scene and its reference, computed once per process and not modified by the tests that share it."""
    if key not in _REF:
        scene = builder()
        _REF[key] = (scene,) + reference(scene)
    return _REF[key]
