"""K13: the geometry pass (geometry_pass.glsl through GPU_OpDrawIndexed) on the GPU against the CPU reference of the contract
(tests/geometry_raster_ref.py).  Depth, normal, ORM, emissive and velocity are compared bit for bit; base colour
within one 8-bit code (hardware pow).  Every frame is at most 193 x 97 with a few hundred triangles and 32^2 textures."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_raster_ref as G  # noqa: E402
import sun_raster_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF
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


class Rig:
    """G-buffer, post-process (for the velocity targets), geometry pass, materials and one single-part PBR_Mesh per draw of a scene."""

    def __init__(self, L, scene):
        import pbrhip
        self.L, self.scene = L, scene
        W, H = scene["W"], scene["H"]
        self.gb = pbrhip.PBR_GBuffer()
        L.PBR_MakeGBuffer(C.byref(self.gb), W, H, pbrhip.Format_RGBA16F)
        self.pp = L.PBR_MakePostProcess(C.byref(self.gb), W, H, pbrhip.Format_RGBA8UN)
        self.gp = L.PBR_MakeGeometryPass(C.byref(self.gb), self.pp, W, H)
        assert self.gp
        self.mats = [pbrhip.make_material(m) for m in scene["materials"]]
        self.meshes = []
        for ps in scene["passes"]:
            for d in ps["draws"]:
                v, ix = scene["meshes"][d["mesh"]]
                mesh = pbrhip.make_mesh(v, ix, [(d["first_index"], d["index_count"])])
                L.PBR_MeshSetPartMaterial(mesh, 0, self.mats[d["material"]])
                self.meshes.append(mesh)
        self.bufs = []

    def globals_of(self, d):
        import pbrhip
        g = pbrhip.PBR_Globals()
        for k in range(16):
            g.clip_space_from_world[k] = float(d["m"][k])
            g.old_clip_space_from_world[k] = float(d["m_old"][k])
        return g

    def write_globals(self, d):
        glob = self.globals_of(d)                                             # kept alive across the copy
        C.memmove(self.L.PBR_GeometryGlobalsBuffer(self.gp).contents.data, C.addressof(glob), C.sizeof(glob))

    def record(self, g, frame_idx=0, write_globals=True):
        """One PBR_RecordGeometryPass per pass of the scene when it has one draw; else the raw call sequence (draws of one pass share
        a render-pass instance, each with its own set, buffers and pushed jitter)."""
        import pbrhip
        L, k = self.L, 0
        for ps in self.scene["passes"]:
            draws = ps["draws"]
            d0 = draws[0]
            if write_globals:
                self.write_globals(d0)
            if ps["clear"]:
                L.GPU_OpClearDepthStencil(g, self.gb.depth, ALL)
            L.GPU_OpPrepareRenderPass(g, L.PBR_GeometryRenderPass(self.gp, frame_idx))
            params = [L.GPU_OpPrepareDrawParams(g, L.PBR_GeometryPipeline(self.gp, frame_idx), L.PBR_GeometryDescriptorSet(self.gp, self.mats[d["material"]]))
                      for d in draws]
            L.GPU_OpBeginRenderPass(g)
            for p, d in zip(params, draws):
                mesh = self.meshes[k]
                k += 1
                L.GPU_OpBindVertexBuffer(g, L.PBR_MeshVertexBuffer(mesh))
                L.GPU_OpBindIndexBuffer(g, L.PBR_MeshIndexBuffer(mesh))
                push = (C.c_float * 4)(*d["jitter"], *d["jitter_prev"])
                L.GPU_OpPushGraphicsConstants(g, L.PBR_GeometryLayout(self.gp), push, 16)
                L.GPU_OpBindDrawParams(g, p)
                L.GPU_OpDrawIndexed(g, d["index_count"], 1, d["first_index"], d["vertex_offset"], 0)
            L.GPU_OpEndRenderPass(g)

    def read(self, frame_idx=0):
        import pbrhip
        gb = self.gb
        return dict(base=pbrhip.read_mip(gb.base_color, 0), nrm=pbrhip.read_mip(gb.normal, 0), orm=pbrhip.read_mip(gb.orm, 0),
                    emi=pbrhip.read_mip(gb.emissive, 0), vel=pbrhip.read_mip(self.L.PBR_PostVelocity(self.pp, frame_idx), 0),
                    depth=pbrhip.read_mip(gb.depth, 0)[..., 0].copy())

    def clear_colour(self, g):
        for t in (self.gb.base_color, self.gb.normal, self.gb.orm, self.gb.emissive, self.L.PBR_PostVelocity(self.pp, 0)):
            self.L.GPU_OpClearColorF(g, t, ALL, 0.0, 0.0, 0.0, 0.0)

    def destroy(self):
        L = self.L
        for m in self.meshes:
            L.PBR_DestroyMesh(m)
        L.PBR_DestroyGeometryPass(self.gp)
        for m in self.mats:
            L.PBR_DestroyMaterial(m)
        L.PBR_DestroyPostProcess(self.pp); L.PBR_DestroyGBuffer(C.byref(self.gb))


def check(name, got, want):
    for key in ("depth", "nrm", "orm", "emi", "vel"):
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
        bad = int((a.view(bits) != b.view(bits)).sum())
        print(f"{name}: {key}: {bad} differing values / tolerance 0 (bit-identical)")
        assert bad == 0, (name, key, bad, np.argwhere(a.view(bits) != b.view(bits))[:5].tolist())
    d = np.abs(got["base"].astype(np.int32) - want["base"].astype(np.int32)).max()
    print(f"{name}: base colour: worst difference {d} codes / tolerance 1 (hardware pow)")
    assert d <= 1


_REF = {}


def ref_of(key, builder):
    if key not in _REF:
        scene = builder()
        _REF[key] = (scene,) + reference(scene)
    return _REF[key]


def run(L, scene, host_sequence=False):
    rig = Rig(L, scene)
    g = L.GPU_MakeGraph()
    before = L.GPUX_RasterRejectedTriangles()
    if host_sequence:                                                        # host/pbr_geometry.c's restatement of render.cpp:993, :1076-1115
        d = scene["passes"][0]["draws"][0]
        glob = rig.globals_of(d)
        L.PBR_RecordGeometryPass(rig.gp, g, rig.meshes[0], None, C.byref(glob), (C.c_float * 2)(*d["jitter"]), (C.c_float * 2)(*d["jitter_prev"]), 0)
    else:
        rig.record(g)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    got = rig.read()
    rejected = L.GPUX_RasterRejectedTriangles() - before
    L.GPU_DestroyGraph(g)
    rig.destroy()
    return got, rejected


def test_geometry_tie_grid_64(gpu):
    scene, want, wins, rej = ref_of("tie", tie_grid_scene)
    assert rej == 0 and (wins[0] >= 0).all()                                 # every pixel is won, once: one winner per pixel
    got, rejected = run(gpu, scene, host_sequence=True)
    assert rejected == 0
    check("tie grid 64^2", got, want)
    # every won pixel names its triangle twice: by its depth and by its flat emissive colour
    d = scene["passes"][0]["draws"][0]
    zs = d["vertices"][0::3, 2]
    won = wins[0] >= 0
    assert np.array_equal(got["depth"][won], zs[wins[0][won]])
    k = wins[0][won]
    emi = np.stack([k % 256, k // 256 * 16 + 7, (k * 7) % 256, np.full_like(k, 255)], -1).astype(np.uint8)
    assert np.array_equal(got["emi"][won], emi)


def test_geometry_random_triangles_64x48(gpu):
    scene, want, wins, rej = ref_of("random", random_scene)
    assert rej >= 2 and 0.2 < (wins[0] >= 0).mean() < 1.0
    got, rejected = run(gpu, scene)
    print(f"rejected: GPU {rejected}, reference {rej}")
    assert rejected == rej
    check("random 64x48", got, want)


def test_geometry_two_draws_and_second_pass_without_clear(gpu):
    scene, want, wins, rej = ref_of("two", two_draw_scene)
    assert (wins[1] >= 0).mean() > 0.01                                      # the second pass won pixels on the first's depth
    got, rejected = run(gpu, scene)
    assert rejected == rej
    check("two draws, two passes 64x40", got, want)


def test_geometry_odd_size_33x17(gpu):
    scene, want, wins, rej = ref_of("odd", lambda: random_scene(33, 17, 150, seed=0x5EED1306))
    assert (wins[0][:, 32] >= 0).any() and (wins[0][16] >= 0).any()          # the cut quads of the last column and row are hit
    got, rejected = run(gpu, scene)
    assert rejected == rej
    check("odd size 33x17", got, want)


@pytest.mark.parametrize("W,H", [(192, 96), (193, 97)])
def test_geometry_second_batch_and_large_list(gpu, W, H):
    """What no other frame of this file reaches (none has more than six tiles; profiles/raster_shared.md lists each frame's load): a
    record on the large list, its box touching all 18 or 28 tiles.  Beside it a bin of more than 256 records, walked in two batches,
    which only the end-to-end frame has otherwise; at 193 x 97 with a last tile column and row one pixel wide.  No pixel is left out
    of the comparison."""
    scene, want, wins, rej = ref_of(("crowded", W, H), lambda: crowded_scene(W, H))
    bins, large = R.tile_load(scene["tris"], W, H)
    assert bins.max() > 256 and large >= 1 and bins[:, -1].max() >= 1 and bins[-1, :].max() >= 1
    assert rej == 0 and (wins[0] >= 0).all() and len(np.unique(wins[0])) > 200      # nothing rejected, every pixel won, most triangles seen
    got, rejected = run(gpu, scene)
    assert rejected == 0                                                     # the counter does not move
    check(f"crowded {W}x{H}", got, want)


def test_geometry_replay_overlap_and_globals_snapshot(gpu):
    L = gpu
    scene, want, wins, rej = ref_of("odd", lambda: random_scene(33, 17, 150, seed=0x5EED1306))
    rig = Rig(L, scene)
    graphs = [L.GPU_MakeGraph(), L.GPU_MakeGraph()]
    try:
        for replay in (0, 1):
            for overlap in (0, 1):
                L.GPUX_SetGraphReplay(replay); L.GPUX_SetGraphOverlap(overlap)
                for f in range(3):
                    g = graphs[f % 2]
                    rig.clear_colour(g)
                    rig.record(g)
                    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
                    check(f"replay {replay} overlap {overlap} frame {f}", rig.read(), want)
        # Globals rewritten between recording and submit: the pass uses what the buffer holds at submit
        g = graphs[0]
        d0 = scene["passes"][0]["draws"][0]
        rig.clear_colour(g)
        rig.write_globals(dict(d0, m=perspective(33, 17, eye=(3.0, 0.0, 0.0))))  # another camera while recording
        rig.record(g, write_globals=False)
        rig.write_globals(d0)                                                 # after recording, before submitting
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        check("Globals rewritten before submit", rig.read(), want)
    finally:
        L.GPUX_SetGraphReplay(-1); L.GPUX_SetGraphOverlap(-1)
    for g in graphs:
        L.GPU_DestroyGraph(g)
    rig.destroy()


class _Errors:
    def __init__(self, L):
        self.L, self.msgs = L, []
        self.cb = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)(lambda m, u: self.msgs.append(m.decode()))

    def __enter__(self):
        self.L.GPUX_SetErrorHandler(C.cast(self.cb, C.c_void_p), None)
        return self.msgs

    def __exit__(self, *a):
        self.L.GPUX_SetErrorHandler(None, None)


def test_geometry_misuse_reports_and_launches_nothing(gpu):
    import pbrhip
    L = gpu
    scene, want, wins, rej = ref_of("odd", lambda: random_scene(33, 17, 150, seed=0x5EED1306))
    W, H = scene["W"], scene["H"]
    rig = Rig(L, scene)
    g = L.GPU_MakeGraph()
    rig.record(g)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    base = rig.read()

    def desc(**kw):
        path = b"shaders/geometry_pass.glsl"
        d = pbrhip.GPU_GraphicsPipelineDesc()
        d.layout = kw.get("layout", L.PBR_GeometryLayout(rig.gp)); d.render_pass = kw.get("render_pass", L.PBR_GeometryRenderPass(rig.gp, 0))
        d.vs.glsl_debug_filepath = pbrhip.GPU_String(path, len(path)); d.fs.glsl_debug_filepath = d.vs.glsl_debug_filepath
        fmts = (C.c_int * 4)(pbrhip.Format_RGB32F, pbrhip.Format_RGB32F, pbrhip.Format_RGB32F, pbrhip.Format_RG32F)
        d.vertex_input_formats = C.cast(fmts, C.POINTER(C.c_int)); d.vertex_input_formats_count = 4
        d.enable_depth_test = True; d.enable_depth_write = True
        d.enable_blending = kw.get("blend", False); d.cull_mode = kw.get("cull", pbrhip.CullMode_DrawCCW)
        return d, fmts

    d, keep = desc()
    ok = L.GPU_MakeGraphicsPipeline(C.byref(d))
    assert ok
    L.GPU_DestroyGraphicsPipeline(ok)
    gb = rig.gb
    vel = L.PBR_PostVelocity(rig.pp, 0)

    def make_pass(texs):
        views = (pbrhip.GPU_TextureView * len(texs))(*[pbrhip.GPU_TextureView(t, 0) for t in texs])
        rd = pbrhip.GPU_RenderPassDesc()
        rd.color_targets_count = len(texs); rd.color_targets = views; rd.width = W; rd.height = H; rd.depth_stencil_target = gb.depth
        return L.GPU_MakeRenderPass(C.byref(rd)), views

    four, k1 = make_pass([gb.base_color, gb.normal, gb.orm, gb.emissive])
    wrong_fmt, k2 = make_pass([gb.base_color, gb.normal, gb.orm, vel, gb.emissive])
    with _Errors(L) as msgs:
        for kw in ({"render_pass": four}, {"render_pass": wrong_fmt}, {"blend": True}, {"cull": pbrhip.CullMode_TwoSided}):
            n = len(msgs)
            d, keep = desc(**kw)
            assert not L.GPU_MakeGraphicsPipeline(C.byref(d)), kw
            assert len(msgs) == n + 1, (kw, msgs[n:])
        # GPU_OpDraw inside the pass
        n = len(msgs)
        L.GPU_OpPrepareRenderPass(g, L.PBR_GeometryRenderPass(rig.gp, 0))
        p = L.GPU_OpPrepareDrawParams(g, L.PBR_GeometryPipeline(rig.gp, 0), L.PBR_GeometryDescriptorSet(rig.gp, rig.mats[0]))
        L.GPU_OpBeginRenderPass(g)
        L.GPU_OpBindDrawParams(g, p)
        L.GPU_OpDraw(g, 3, 1, 0, 0)
        assert len(msgs) == n + 1 and "unsupported (raster)" in msgs[-1], msgs[n:]
        # a descriptor set with a texture binding left out
        s = L.GPU_InitDescriptorSet(None, L.PBR_GeometryLayout(rig.gp))
        L.GPU_SetBufferBinding(s, 0, L.PBR_GeometryGlobalsBuffer(rig.gp))
        for b in (1, 2, 4):
            L.GPU_SetTextureBinding(s, b, L.PBR_MaterialTexture(rig.mats[0], 0))
        L.GPU_SetSamplerBinding(s, 5, L.GPU_SamplerLinearWrap())
        n = len(msgs)
        L.GPU_FinalizeDescriptorSet(s)
        assert len(msgs) == n + 1 and "TEX_ORM" in msgs[-1], msgs[n:]
        L.GPU_OpEndRenderPass(g)
        n = len(msgs)
        L.GPU_OpPrepareRenderPass(g, L.PBR_GeometryRenderPass(rig.gp, 0))
        L.GPU_OpPrepareDrawParams(g, L.PBR_GeometryPipeline(rig.gp, 0), s)         # an unfinalised set cannot be drawn with
        assert len(msgs) == n + 1, msgs[n:]
        L.GPU_OpBeginRenderPass(g)
        L.GPU_OpEndRenderPass(g)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    got = rig.read()
    for key in base:
        assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint8), np.ascontiguousarray(base[key]).view(np.uint8)), key
    # mip generation: non-power-of-two RGBA8UN with mips still fails; the power-of-two chain equals the reference's
    with _Errors(L) as msgs:
        img = np.zeros((12, 12, 4), np.uint8)
        t = L.GPU_MakeTexture(pbrhip.Format_RGBA8UN, 12, 12, 1, pbrhip.TextureFlag_HasMipmaps, img.ctypes.data_as(C.c_void_p))
        assert len(msgs) == 1 and "mip generation" in msgs[0]
        if t:
            L.GPU_DestroyTexture(t)
    chain = G.mip_chain(scene["materials"][0][0])
    tex = L.PBR_MaterialTexture(rig.mats[0], 0)
    assert tex.contents.mip_level_count == len(chain) == 6
    for l, want_l in enumerate(chain):
        assert np.array_equal(pbrhip.read_mip(tex, l), want_l), l
    L.GPU_DestroyDescriptorSet(s); L.GPU_DestroyRenderPass(four); L.GPU_DestroyRenderPass(wrong_fmt)
    L.GPU_DestroyGraph(g)
    rig.destroy()


def test_sun_pass_unchanged_beside_the_geometry_pass(gpu):
    """The sun-depth pipeline is still accepted and bit-identical on one K12 fixture (a small random map)."""
    import pbrhip
    L = gpu
    W = 64
    rng = np.random.default_rng(0x5EED1307)
    n = 400
    c = rng.uniform(-8, W + 8, (n, 1, 2))
    v = c + rng.normal(size=(n, 3, 2)) * np.exp(rng.uniform(np.log(0.2), np.log(40.0), (n, 1, 1)))
    pos = np.concatenate([v, rng.uniform(-0.1, 1.1, (n, 3, 1))], 2).reshape(-1, 3).astype(f32)
    idx = np.arange(3 * n, dtype=np.uint32)
    M = R.pixel_matrix(W, W)
    glob = pbrhip.PBR_Globals()
    for k in range(16):
        glob.sun_space_from_world[k] = float(M[k])
    sp = L.PBR_MakeSunDepthPass(W)
    mesh = pbrhip.make_mesh(pos, idx, [(0, 3 * n)])
    g = L.GPU_MakeGraph()
    L.PBR_RecordSunDepthPass(sp, g, mesh, C.byref(glob))
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    got = pbrhip.read_mip(L.PBR_SunDepthTexture(sp), 0)[..., 0]
    want, _ = R.raster(np.ones((W, W), f32), pos, idx, [(3 * n, 1, 0, 0, M)])
    assert (want < 1).mean() > 0.5
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    L.GPU_DestroyGraph(g); L.PBR_DestroyMesh(mesh); L.PBR_DestroySunDepthPass(sp)


def test_geometry_end_to_end_sun_depth_geometry_lighting_96x54(gpu):
    """One graph: sun depth (K12) -> geometry (K13) -> lighting (K5, IBL mode with sun shadows) over synth_mesh_temple(3000) with four
    materials, against the same chain on the CPU: the reference G-buffer and the reference sun map through the lighting oracle, at the
    tolerance of the 96 x 54 lighting tests (relative 1e-4, floor 1e-2)."""
    import pbrhip, pbr_oracle as O
    from pbrhip import synth
    L = gpu
    W, H = 96, 54
    verts, idx, parts, part_mat = synth.synth_mesh_temple(3000, n_materials=4)
    rng = np.random.default_rng(0x5EED1308)
    verts = verts.copy()
    verts[:, 3:6] = rng.normal(size=(len(verts), 3)) * 0.2 + (0.0, 0.0, 1.0)  # bumpy normals
    mats = synth.synth_materials(4, 32, seed=0x5EED1309)
    env = synth.synth_env(64, seed=0x5EED00AA)
    env_tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 64, 64, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), 16, 64, 32)
    L.PBR_GenIrradianceMap(env_tex, maps.irradiance_map); L.PBR_GenPrefilteredEnvMap(env_tex, maps.tex_specular_env_map, 1); L.PBR_GenBRDFIntegrationMap(maps.brdf_lut)
    gb = pbrhip.PBR_GBuffer()
    L.PBR_MakeGBuffer(C.byref(gb), W, H, pbrhip.Format_RGBA32F)
    pp = L.PBR_MakePostProcess(C.byref(gb), W, H, pbrhip.Format_RGBA8UN)
    gp = L.PBR_MakeGeometryPass(C.byref(gb), pp, W, H)
    sp = L.PBR_MakeSunDepthPass(256)
    materials = [pbrhip.make_material(m) for m in mats]
    mesh = pbrhip.make_mesh(verts, idx, parts)
    for k, m in enumerate(part_mat):
        L.PBR_MeshSetPartMaterial(mesh, k, materials[m])
    lp = L.PBR_MakeLightingPassEx(C.byref(gb), C.byref(maps), W, H, L.PBR_SunDepthTexture(sp))
    L.GPUX_SetShadeFlags(L.PBR_LightingPipeline(lp), pbrhip.Shade_IBL | pbrhip.Shade_SunShadows)
    frame = 1                                                                # the odd velocity target
    glob = pbrhip.fill_globals((0.0, -30.0, 6.0), aspect=W / H, frame_idx=frame)
    old = pbrhip.fill_globals((0.2, -30.1, 6.0), aspect=W / H)
    for k in range(16):
        glob.old_clip_space_from_world[k] = old.clip_space_from_world[k]
    jit, jp = (0.3 / W, -0.2 / H), (-0.1 / W, 0.25 / H)
    g = L.GPU_MakeGraph()
    L.PBR_RecordSunDepthPass(sp, g, mesh, C.byref(glob))
    L.PBR_RecordGeometryPass(gp, g, mesh, None, C.byref(glob), (C.c_float * 2)(*jit), (C.c_float * 2)(*jp), frame)
    L.PBR_RecordLightingPass(lp, g, C.byref(glob), 0, 0)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    got = dict(base=pbrhip.read_mip(gb.base_color, 0), nrm=pbrhip.read_mip(gb.normal, 0), orm=pbrhip.read_mip(gb.orm, 0), emi=pbrhip.read_mip(gb.emissive, 0),
               vel=pbrhip.read_mip(L.PBR_PostVelocity(pp, frame), 0), depth=pbrhip.read_mip(gb.depth, 0)[..., 0].copy())
    lit = pbrhip.read_mip(gb.lighting_result, 0)
    assert not pbrhip.read_mip(L.PBR_PostVelocity(pp, 0), 0).any()           # the other velocity target is untouched
    # the same chain on the CPU
    M, Mo = np.array(list(glob.clip_space_from_world), f32), np.array(list(glob.old_clip_space_from_world), f32)
    chains = [[G.mip_chain(im) for im in m] for m in mats]
    draws = [dict(m=M, m_old=Mo, jitter=jit, jitter_prev=jp, material=chains[part_mat[k]], vertices=verts, indices=idx, index_count=c, first_index=f, vertex_offset=0)
             for k, (f, c) in enumerate(parts)]
    t0 = dict(base=np.zeros((H, W, 4), np.uint8), nrm=np.zeros((H, W, 4), np.uint8), orm=np.zeros((H, W, 4), np.uint8),
              emi=np.zeros((H, W, 4), np.uint8), vel=np.zeros((H, W, 2), np.float16), depth=np.ones((H, W), f32))
    want, win, rej = G.raster(t0, draws)
    assert 0.3 < (win >= 0).mean() < 0.9 and len(np.unique(win)) > 300            # temple and sky both in the frame
    check("end to end 96x54: G-buffer", got, want)
    sun_map, _ = R.raster(np.ones((256, 256), f32), verts[:, :3], idx, [(c, 1, f, 0, np.array(list(glob.sun_space_from_world), f32)) for f, c in parts])
    assert np.array_equal(pbrhip.read_mip(L.PBR_SunDepthTexture(sp), 0)[..., 0].view(np.uint32), sun_map.view(np.uint32))
    irr = pbrhip.read_mip(maps.irradiance_map, 0)
    nm = maps.tex_specular_env_map.contents.mip_level_count
    pyr = np.concatenate([pbrhip.read_mip(maps.tex_specular_env_map, m).ravel() for m in range(nm)])
    og = O.OrcGlobals.from_buffer_copy(bytes(glob))
    ref = O.shade(og, want["base"], want["nrm"], want["orm"], want["emi"], want["depth"], flags=O.SHADE_IBL | O.SHADE_SHADOWS, irradiance_cube=irr,
                  prefiltered_pyr=pyr, prefiltered_size=maps.tex_specular_env_map.contents.width,
                  lut_half=pbrhip.read_mip(maps.brdf_lut, 0).view(np.uint16), sun_depth_map=sun_map)
    err = np.abs(lit[..., :3].astype(np.float64) - ref[..., :3]) / np.maximum(np.abs(ref[..., :3]), 1e-2)
    print(f"end to end 96x54: lighting of the rasterised G-buffer: worst relative error {err.max():.3g} / tolerance 1e-4")
    assert err.max() < 1e-4
    L.GPU_DestroyGraph(g); L.PBR_DestroyLightingPass(lp); L.PBR_DestroyMesh(mesh); L.PBR_DestroySunDepthPass(sp); L.PBR_DestroyGeometryPass(gp)
    for m in materials:
        L.PBR_DestroyMaterial(m)
    L.PBR_DestroyPostProcess(pp); L.PBR_DestroyGBuffer(C.byref(gb)); L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(env_tex)
