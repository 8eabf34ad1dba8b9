"""N5 / K12: the sun depth pass (sun_depth_pass.glsl through GPU_OpDrawIndexed) on the GPU against the CPU reference of the contract
(tests/sun_raster_ref.py).  Maps are compared bit for bit; each test prints its worst difference and tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sun_raster_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF


def _globals(M):
    import pbrhip
    g = pbrhip.PBR_Globals()
    for k in range(16):
        g.sun_space_from_world[k] = float(M[k])
    return g


def _sun_matrix(glob):
    return np.array(list(glob.sun_space_from_world), np.float32)


def _write_globals(buf, glob):
    C.memmove(buf.contents.data, C.addressof(glob), C.sizeof(glob))


def _extra_set(L, sp, M):
    """A second descriptor set of the sun pass's layout with a mapped Globals buffer of its own."""
    import pbrhip
    buf = L.GPU_MakeBuffer(C.sizeof(pbrhip.PBR_Globals) + 8, pbrhip.BufferFlag_CPU | pbrhip.BufferFlag_GPU | pbrhip.BufferFlag_StorageBuffer, None)
    _write_globals(buf, _globals(M))
    s = L.GPU_InitDescriptorSet(None, L.PBR_SunDepthLayout(sp))
    L.GPU_SetBufferBinding(s, 0, buf)
    L.GPU_FinalizeDescriptorSet(s)
    return s, buf


def _record(L, g, sp, mesh, draws, clear=True, vb=True, ib=True):
    """The reference's call sequence (render.cpp:995-1020); draws: [(set, index_count, instance_count, first_index, vertex_offset)]."""
    if clear:
        L.GPU_OpClearDepthStencil(g, L.PBR_SunDepthTexture(sp), ALL)
    L.GPU_OpPrepareRenderPass(g, L.PBR_SunDepthRenderPass(sp))
    params = [L.GPU_OpPrepareDrawParams(g, L.PBR_SunDepthPipeline(sp), d[0]) for d in draws]
    L.GPU_OpBeginRenderPass(g)
    if vb:
        L.GPU_OpBindVertexBuffer(g, L.PBR_MeshVertexBuffer(mesh))
    if ib:
        L.GPU_OpBindIndexBuffer(g, L.PBR_MeshIndexBuffer(mesh))
    for p, d in zip(params, draws):
        L.GPU_OpBindDrawParams(g, p)
        L.GPU_OpDrawIndexed(g, d[1], d[2], d[3], d[4], 0)
    L.GPU_OpEndRenderPass(g)


def _map(L, sp):
    import pbrhip
    return pbrhip.read_mip(L.PBR_SunDepthTexture(sp), 0)[..., 0].copy()


def _check(name, got, want):
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    nbits = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{name}: worst |diff| {diff.max():.3g} over {nbits} texels / tolerance 0 (bit-identical); {float((want < 1).mean()):.3f} of the map covered")
    assert nbits == 0, (name, nbits, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5].tolist())


class _Errors:
    def __init__(self, L):
        self.L, self.msgs = L, []
        self.cb = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)(lambda m, u: self.msgs.append(m.decode()))

    def __enter__(self):
        self.L.GPUX_SetErrorHandler(C.cast(self.cb, C.c_void_p), None)
        return self.msgs

    def __exit__(self, *a):
        self.L.GPUX_SetErrorHandler(None, None)


def test_sun_depth_tie_grid_64(gpu):
    """Warped grid of quads with every vertex on a pixel centre, plus an overlapping fan layer; each triangle has its own constant
    depth, so every texel names the lowest triangle whose coverage (top-left rule) holds its centre."""
    import pbrhip
    L = gpu
    W = 64
    rng = np.random.default_rng(0x5EED1201)
    n = 8
    P = np.zeros((n + 1, n + 1, 2))
    for a in range(n + 1):
        for b in range(n + 1):
            jit = rng.integers(-2, 3, 2) if 0 < a < n and 0 < b < n else (0, 0)
            P[a, b] = (8 * a + jit[0], 8 * b + jit[1])
    P = np.minimum(P, W - 1) + 0.5
    tris = []
    for a in range(n):
        for b in range(n):
            p00, p10, p01, p11 = P[a, b], P[a + 1, b], P[a, b + 1], P[a + 1, b + 1]
            tris += [[p00, p10, p11], [p00, p11, p01]] if rng.random() < 0.5 else [[p00, p10, p01], [p10, p11, p01]]
    hub = np.array([32.5, 32.5])
    rim = [np.array(v) + 0.5 for v in ((10, 10), (32, 4), (54, 10), (60, 32), (54, 54), (32, 60), (10, 54), (4, 32), (10, 10))]
    tris += [[hub, rim[k], rim[k + 1]] for k in range(8)]
    tris += [[rng.integers(0, W, 2) + 0.5 for _ in range(3)] for _ in range(40)]
    tris = np.array(tris, np.float64)
    m = len(tris)
    depth = (rng.permutation(m) + 1).astype(np.float64) / (m + 2)
    pos = np.concatenate([tris.reshape(-1, 2), np.repeat(depth, 3)[:, None]], 1).astype(np.float32)
    idx = np.arange(3 * m, dtype=np.uint32)
    M = R.pixel_matrix(W, W)
    sp = L.PBR_MakeSunDepthPass(W)
    mesh = pbrhip.make_mesh(pos, idx, [(0, 3 * m)])
    g = L.GPU_MakeGraph()
    L.PBR_RecordSunDepthPass(sp, g, mesh, C.byref(_globals(M)))
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    want, rej = R.raster(np.ones((W, W), np.float32), pos, idx, [(3 * m, 1, 0, 0, M)])
    assert rej == 0 and (want < 1).mean() > 0.9
    _check("tie grid 64^2", _map(L, sp), want)
    L.GPU_DestroyGraph(g); L.PBR_DestroyMesh(mesh); L.PBR_DestroySunDepthPass(sp)


def test_sun_depth_random_256(gpu):
    """~20k random triangles from sub-pixel to larger than the viewport, with degenerate, NaN, guard-band, out-of-range-index and
    partly-outside-[0,1] ones; several draws with first_index / vertex_offset != 0, instance counts 0 and 3, a ragged index count;
    a second pass in the same graph onto the same map with pose 2's matrix (w = 1.0000001) from its own Globals buffer."""
    import pbrhip
    L = gpu
    W = 256
    rng = np.random.default_rng(0x5EED1202)
    n = 20000
    c = rng.uniform(-64, W + 64, (n, 1, 2))
    size = np.exp(rng.uniform(np.log(0.1), np.log(600.0), (n, 1, 1)))
    v = c + rng.normal(size=(n, 3, 2)) * size
    z = rng.uniform(-0.2, 1.2, (n, 3))
    q = n // 100
    v[0:q, 1] = v[0:q, 0]                                                   # degenerate: repeated vertex
    v[q:2 * q, 2] = v[q:2 * q, 0] + 2.0 * (v[q:2 * q, 1] - v[q:2 * q, 0])  # degenerate: collinear (zero area unless rounding says otherwise)
    pa = np.concatenate([v, z[..., None]], 2).reshape(-1, 3).astype(np.float32)
    pa[3 * (2 * q):3 * (2 * q) + 3 * q:3, 0] = np.nan                       # NaN
    pa[3 * (3 * q) + 1:3 * (4 * q):3, 1] = 3.0e6                            # outside the guard band
    pa[3 * (4 * q) + 2:3 * (5 * q):3, 2] = np.inf                           # infinite depth
    # world-space block for the second pass (pose 2: sun angle (20, 200), sun_space_from_world[15] = 1.0000001)
    glob2 = pbrhip.fill_globals((0.0, 0.0, 0.0), sun_angle=(20.0, 200.0))
    M2 = _sun_matrix(glob2)
    assert M2[15] == np.float32(1.0000001)
    m2 = 3000
    wc = rng.uniform(-45, 45, (m2, 1, 3))
    pw = (wc + rng.normal(size=(m2, 3, 3)) * np.exp(rng.uniform(np.log(0.05), np.log(8.0), (m2, 1, 1)))).reshape(-1, 3).astype(np.float32)
    pos = np.concatenate([pa, pw])
    nva = len(pa)
    # index buffer: [A0: tris 0..n/2 as is][A1: the rest, stored minus 100][bad indices][B: world block, relative to nva]
    ia = np.arange(3 * n, dtype=np.int64)
    h = 3 * (n // 2)
    bad = np.array([0, 1, len(pos) + 5, 2, len(pos) + 1000, 4], np.int64)
    ib = np.arange(3 * m2, dtype=np.int64)
    idx = np.concatenate([ia[:h], ia[h:] - 100, bad, ib]).astype(np.uint32)
    fa1, fbad, fb = h, 3 * n, 3 * n + len(bad)
    M = R.pixel_matrix(W, W)
    sp = L.PBR_MakeSunDepthPass(W)
    s0 = L.PBR_SunDepthDescriptorSet(sp)
    _write_globals(L.PBR_SunDepthGlobalsBuffer(sp), _globals(M))
    s2, buf2 = _extra_set(L, sp, M2)
    mesh = pbrhip.make_mesh(pos, idx, [])
    draws_a = [(s0, h, 1, 0, 0), (s0, 3 * n - h + 2, 3, fa1, 100), (s0, len(bad), 1, fbad, 0), (s0, 3 * n, 0, 0, 0)]
    draws_b = [(s2, 3 * m2 // 2, 1, fb, nva), (s2, 3 * m2 - 3 * (m2 // 2), 1, fb + 3 * (m2 // 2), nva)]
    before = L.GPUX_RasterRejectedTriangles()
    g = L.GPU_MakeGraph()
    _record(L, g, sp, mesh, draws_a)
    _record(L, g, sp, mesh, draws_b, clear=False)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    rejected = L.GPUX_RasterRejectedTriangles() - before
    got = _map(L, sp)
    mid, rej_a = R.raster(np.ones((W, W), np.float32), pos, idx, [(d[1], d[2], d[3], d[4], M) for d in draws_a])
    want, rej_b = R.raster(mid, pos, idx, [(d[1], d[2], d[3], d[4], M2) for d in draws_b])
    print(f"rejected: GPU {rejected}, reference {rej_a + rej_b}")
    assert rej_a >= 3 * q + 2 and rejected == rej_a + rej_b
    assert (want < mid).mean() > 0.002                                      # the second pass changed the map
    _check("random 256^2, two passes", got, want)
    L.GPU_DestroyGraph(g); L.PBR_DestroyMesh(mesh); L.GPU_DestroyDescriptorSet(s2); L.GPU_DestroyBuffer(buf2)
    L.PBR_DestroySunDepthPass(sp)


def test_sun_depth_second_batch_large_list_and_cut_edge_tiles_193x97(gpu):
    """A 193 x 97 map (7 x 4 tiles, the last column and row one pixel wide) through the raw call sequence on a depth target of its own:
    a triangle over the whole map (large list), 260 single-tile ones in one bin (a second batch of 256) and six across the right and
    bottom edges.  The other maps of this file are square multiples of the tile; every texel is compared."""
    import pbrhip
    L = gpu
    W, H = 193, 97
    tris, depth = R.crowded_triangles(W, H)
    bins, large = R.tile_load(tris, W, H)
    assert bins.max() > 256 and large >= 1 and bins[:, -1].max() >= 1 and bins[-1, :].max() >= 1
    m = len(tris)
    pos = np.concatenate([tris.reshape(-1, 2), np.repeat(depth, 3)[:, None]], 1).astype(np.float32)
    idx = np.arange(3 * m, dtype=np.uint32)
    M = R.pixel_matrix(W, H)
    want, rej = R.raster(np.ones((H, W), np.float32), pos, idx, [(3 * m, 1, 0, 0, M)])
    assert rej == 0 and (want < 1).all()                                    # the reference rejects nothing and covers every texel
    sp = L.PBR_MakeSunDepthPass(64)                                         # for its layout, descriptor set and Globals buffer
    tex = pbrhip.make_texture(pbrhip.Format_D32F_Or_X8D24UN, W, H, pbrhip.TextureFlag_RenderTarget)
    rd = pbrhip.GPU_RenderPassDesc()
    rd.color_targets_count = 0; rd.width = W; rd.height = H; rd.depth_stencil_target = tex
    rp = L.GPU_MakeRenderPass(C.byref(rd))
    d, keep = _pipeline_desc(L, sp, render_pass=rp)
    pipe = L.GPU_MakeGraphicsPipeline(C.byref(d))
    assert pipe
    _write_globals(L.PBR_SunDepthGlobalsBuffer(sp), _globals(M))
    mesh = pbrhip.make_mesh(pos, idx, [(0, 3 * m)])
    before = L.GPUX_RasterRejectedTriangles()
    g = L.GPU_MakeGraph()
    L.GPU_OpClearDepthStencil(g, tex, ALL)
    L.GPU_OpPrepareRenderPass(g, rp)
    p = L.GPU_OpPrepareDrawParams(g, pipe, L.PBR_SunDepthDescriptorSet(sp))
    L.GPU_OpBeginRenderPass(g)
    L.GPU_OpBindVertexBuffer(g, L.PBR_MeshVertexBuffer(mesh))
    L.GPU_OpBindIndexBuffer(g, L.PBR_MeshIndexBuffer(mesh))
    L.GPU_OpBindDrawParams(g, p)
    L.GPU_OpDrawIndexed(g, 3 * m, 1, 0, 0, 0)
    L.GPU_OpEndRenderPass(g)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    got = pbrhip.read_mip(tex, 0)[..., 0].copy()
    assert L.GPUX_RasterRejectedTriangles() == before                       # the counter does not move
    _check("crowded 193x97", got, want)
    L.GPU_DestroyGraph(g); L.PBR_DestroyMesh(mesh); L.GPU_DestroyGraphicsPipeline(pipe); L.GPU_DestroyRenderPass(rp)
    L.GPU_DestroyTexture(tex); L.PBR_DestroySunDepthPass(sp)


def test_sun_depth_reference_frame_2048(gpu):
    """PBR_RecordSunDepthPass over synth_mesh_temple (~200k triangles, ~100 parts: one draw per part) at 2048^2, at the default
    sun angle (56.5, 97) and two others."""
    import pbrhip
    from pbrhip import synth
    L = gpu
    verts, idx, parts = synth.synth_mesh_temple(200000)
    assert 90 <= len(parts) <= 110 and len(idx) // 3 > 180000
    sp = L.PBR_MakeSunDepthPass(2048)
    mesh = pbrhip.make_mesh(verts, idx, parts)
    assert L.PBR_MeshPartCount(mesh) == len(parts)
    g = L.GPU_MakeGraph()
    for angle in ((56.5, 97.0), (35.0, 40.0), (80.0, 250.0)):
        glob = pbrhip.fill_globals((0.0, -30.0, 6.0), sun_angle=angle)
        before = L.GPUX_RasterRejectedTriangles()
        L.PBR_RecordSunDepthPass(sp, g, mesh, C.byref(glob))
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        got = _map(L, sp)
        want, rej = R.raster(np.ones((2048, 2048), np.float32), verts[:, :3], idx, [(c, 1, f, 0, _sun_matrix(glob)) for f, c in parts])
        assert L.GPUX_RasterRejectedTriangles() - before == rej
        assert (want < 1).mean() > 0.3 and len(np.unique(want)) > 1000
        _check(f"temple 2048^2 sun {angle}", got, want)
    L.GPU_DestroyGraph(g); L.PBR_DestroyMesh(mesh); L.PBR_DestroySunDepthPass(sp)


def test_sun_pass_feeds_live_lighting(gpu):
    """One graph: the sun pass, then the live lighting pass (SunShadows | LightShafts) reading its map, at 256 x 144 over the
    synthetic GI scene.  The map is the reference's bit for bit; K5's frame equals the oracle fed the reference map (1e-4)."""
    import pbrhip, pbr_oracle as O
    from pbrhip import synth
    L = gpu
    W, H = 256, 144
    gbd, _, _, _ = synth.synth_gi_scene(W, H)
    env = synth.synth_env(64, seed=0x5EED00AA)
    env_tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 64, 64, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), 16, 64, 32)
    L.PBR_GenIrradianceMap(env_tex, maps.irradiance_map); L.PBR_GenPrefilteredEnvMap(env_tex, maps.tex_specular_env_map, 1); L.PBR_GenBRDFIntegrationMap(maps.brdf_lut)
    gb = pbrhip.PBR_GBuffer()
    L.PBR_MakeGBuffer(C.byref(gb), W, H, pbrhip.Format_RGBA32F)
    for name, key in (("base_color", "base"), ("normal", "normal"), ("orm", "orm"), ("emissive", "emissive"), ("depth", "depth")):
        pbrhip.upload_mip(getattr(gb, name), 0, gbd[key])
    verts, idx, parts = synth.synth_mesh_temple(30000, seed=0x5EED1204)
    verts = verts.copy()
    verts[:, :3] *= np.float32(0.2)                                          # the temple shrunk onto the spheres (scene extent 8)
    sp = L.PBR_MakeSunDepthPass(512)
    mesh = pbrhip.make_mesh(verts, idx, parts)
    lp = L.PBR_MakeLightingPassLive(C.byref(gb), C.byref(maps), W, H, L.PBR_SunDepthTexture(sp), None, None)
    L.GPUX_SetShadeFlags(L.PBR_LightingPipeline(lp), pbrhip.Shade_LightShafts | pbrhip.Shade_SunShadows)
    glob = pbrhip.fill_globals(synth.GI_SCENE_CAMERA, aspect=W / H, frame_idx=3)
    g = L.GPU_MakeGraph()
    L.PBR_RecordSunDepthPass(sp, g, mesh, C.byref(glob))
    L.PBR_RecordLightingPass(lp, g, C.byref(glob), 0, 0)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    ref_map, _ = R.raster(np.ones((512, 512), np.float32), verts[:, :3], idx, [(c, 1, f, 0, _sun_matrix(glob)) for f, c in parts])
    _check("sun map 512^2 (end to end)", _map(L, sp), ref_map)
    got = pbrhip.read_mip(gb.lighting_result, 0)
    irr = pbrhip.read_mip(maps.irradiance_map, 0)
    nm = maps.tex_specular_env_map.contents.mip_level_count
    pyr = np.concatenate([pbrhip.read_mip(maps.tex_specular_env_map, m).ravel() for m in range(nm)])
    og = O.OrcGlobals.from_buffer_copy(bytes(glob))
    want = O.shade(og, gbd["base"], gbd["normal"], gbd["orm"], gbd["emissive"], gbd["depth"], flags=O.SHADE_SHAFTS | O.SHADE_SHADOWS,
                   irradiance_cube=irr, prefiltered_pyr=pyr, prefiltered_size=maps.tex_specular_env_map.contents.width,
                   lut_half=pbrhip.read_mip(maps.brdf_lut, 0).view(np.uint16), sun_depth_map=ref_map)
    err = np.abs(got[..., :3].astype(np.float64) - want[..., :3]) / np.maximum(np.abs(want[..., :3]), 1e-2)
    print(f"lighting with the rasterised sun map: worst relative error {err.max():.3g} / tolerance 1e-4")
    assert err.max() < 1e-4
    lit = O.shade(og, gbd["base"], gbd["normal"], gbd["orm"], gbd["emissive"], gbd["depth"], flags=O.SHADE_SHAFTS | O.SHADE_SHADOWS,
                  irradiance_cube=irr, prefiltered_pyr=pyr, prefiltered_size=maps.tex_specular_env_map.contents.width,
                  lut_half=pbrhip.read_mip(maps.brdf_lut, 0).view(np.uint16), sun_depth_map=np.ones((512, 512), np.float32))
    assert (np.abs(lit[..., :3] - want[..., :3]).max(-1) > 1e-3).mean() > 0.01    # the map really shadows part of the frame
    L.GPU_DestroyGraph(g); L.PBR_DestroyLightingPass(lp); L.PBR_DestroyMesh(mesh); L.PBR_DestroySunDepthPass(sp)
    L.PBR_DestroyGBuffer(C.byref(gb)); L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(env_tex)


def test_sun_depth_replay_overlap_and_globals_snapshot(gpu):
    """Four frames on two graphs in flight under every replay x overlap setting give the reference map; rewriting the mapped Globals
    between recording and GPU_GraphSubmit rasterises with the new sun angle (snapshot at submit, as K5)."""
    import pbrhip
    from pbrhip import synth
    L = gpu
    verts, idx, parts = synth.synth_mesh_temple(40000, seed=0x5EED1205)
    S = 512
    sp = L.PBR_MakeSunDepthPass(S)
    mesh = pbrhip.make_mesh(verts, idx, parts)
    ga = pbrhip.fill_globals((0.0, 0.0, 5.0))
    gb_ = pbrhip.fill_globals((0.0, 0.0, 5.0), sun_angle=(30.0, 160.0))
    ref = {k: R.raster(np.ones((S, S), np.float32), verts[:, :3], idx, [(c, 1, f, 0, _sun_matrix(gl)) for f, c in parts])[0]
           for k, gl in (("a", ga), ("b", gb_))}
    graphs = [L.GPU_MakeGraph(), L.GPU_MakeGraph()]
    try:
        for replay in (0, 1):
            for overlap in (0, 1):
                L.GPUX_SetGraphReplay(replay); L.GPUX_SetGraphOverlap(overlap)
                for f in range(4):
                    g = graphs[f % 2]
                    L.PBR_RecordSunDepthPass(sp, g, mesh, C.byref(ga if f % 2 == 0 else gb_))
                    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
                    _check(f"replay {replay} overlap {overlap} frame {f}", _map(L, sp), ref["a" if f % 2 == 0 else "b"])
        g = graphs[0]
        _write_globals(L.PBR_SunDepthGlobalsBuffer(sp), ga)
        L.PBR_RecordSunDepthPass(sp, g, mesh, None)
        _write_globals(L.PBR_SunDepthGlobalsBuffer(sp), gb_)                  # after recording, before submitting
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        _check("Globals rewritten before submit", _map(L, sp), ref["b"])
    finally:
        L.GPUX_SetGraphReplay(-1); L.GPUX_SetGraphOverlap(-1)
    for g in graphs:
        L.GPU_DestroyGraph(g)
    L.PBR_DestroyMesh(mesh); L.PBR_DestroySunDepthPass(sp)


def _timed_names(L, g):
    return [L.GPUX_GraphTimedOpName(g, i).decode() for i in range(L.GPUX_GraphTimedOpCount(g))]


def test_sun_depth_rebound_buffers_split_the_job_64(gpu):
    """Two meshes with vertex / index buffers of their own drawn in one render-pass instance as A's first half, B, A's second half:
    every change of the bound pair starts a new job (three K12.setup / K12.tiles), in order, onto the same map.  Binding the same
    pair again between two draws does not.  Vertices on pixel centres, one depth per triangle, all depths distinct."""
    import pbrhip
    L = gpu
    W, m = 64, 40
    rng = np.random.default_rng(0x5EED1206)
    depth = (rng.permutation(2 * m) + 1).astype(np.float64) / (2 * m + 2)
    pos = [np.concatenate([(rng.integers(0, W, (3 * m, 2)) + 0.5), np.repeat(depth[k * m:(k + 1) * m], 3)[:, None]], 1).astype(np.float32) for k in range(2)]
    idx = np.arange(3 * m, dtype=np.uint32)
    h = 3 * (m // 2)
    M = R.pixel_matrix(W, W)
    ones = np.ones((W, W), np.float32)
    want1, r1 = R.raster(ones, pos[0], idx, [(h, 1, 0, 0, M)])
    want2, r2 = R.raster(want1, pos[1], idx, [(3 * m, 1, 0, 0, M)])
    want3, r3 = R.raster(want2, pos[0], idx, [(3 * m - h, 1, h, 0, M)])
    both, r4 = R.raster(ones, pos[0], idx, [(h, 1, 0, 0, M), (3 * m - h, 1, h, 0, M)])
    assert r1 == r2 == r3 == r4 == 0
    assert (want1 < ones).any() and (want2 < want1).any() and (want3 < want2).any() and (both < want1).any()     # every job shows in the map
    sp = L.PBR_MakeSunDepthPass(W)
    s = L.PBR_SunDepthDescriptorSet(sp)
    _write_globals(L.PBR_SunDepthGlobalsBuffer(sp), _globals(M))
    meshes = [pbrhip.make_mesh(p, idx, [(0, 3 * m)]) for p in pos]
    graphs = [L.GPU_MakeGraph(), L.GPU_MakeGraph()]

    def record(g, steps):
        """steps: (mesh whose pair is bound in front of the draw, index_count, first_index)"""
        L.GPU_OpClearDepthStencil(g, L.PBR_SunDepthTexture(sp), ALL)
        L.GPU_OpPrepareRenderPass(g, L.PBR_SunDepthRenderPass(sp))
        params = [L.GPU_OpPrepareDrawParams(g, L.PBR_SunDepthPipeline(sp), s) for _ in steps]
        L.GPU_OpBeginRenderPass(g)
        for p, (mesh, count, first) in zip(params, steps):
            L.GPU_OpBindVertexBuffer(g, L.PBR_MeshVertexBuffer(mesh))
            L.GPU_OpBindIndexBuffer(g, L.PBR_MeshIndexBuffer(mesh))
            L.GPU_OpBindDrawParams(g, p)
            L.GPU_OpDrawIndexed(g, count, 1, first, 0, 0)
        L.GPU_OpEndRenderPass(g)

    L.GPUX_EnableOpTiming(1)
    try:
        g = graphs[0]
        record(g, [(meshes[0], h, 0), (meshes[1], 3 * m, 0), (meshes[0], 3 * m - h, h)])
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        names = _timed_names(L, g)
        print(f"A half, B, A half: timed ops {names}")
        assert names.count("K12.setup") == 3 and names.count("K12.tiles") == 3, names
        _check("rebound buffers 64^2: three jobs", _map(L, sp), want3)
        g = graphs[1]
        record(g, [(meshes[0], h, 0), (meshes[0], 3 * m - h, h)])
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        names = _timed_names(L, g)
        print(f"A half, the same pair bound again, A half: timed ops {names}")
        assert names.count("K12.setup") == 1 and names.count("K12.tiles") == 1, names
        _check("rebound buffers 64^2: the same pair again is one job", _map(L, sp), both)
    finally:
        L.GPUX_EnableOpTiming(0)
    for g in graphs:
        L.GPU_DestroyGraph(g)
    for mesh in meshes:
        L.PBR_DestroyMesh(mesh)
    L.PBR_DestroySunDepthPass(sp)


def _pipeline_desc(L, sp, **kw):
    import pbrhip
    path = b"shaders/sun_depth_pass.glsl"
    d = pbrhip.GPU_GraphicsPipelineDesc()
    d.layout = L.PBR_SunDepthLayout(sp); d.render_pass = kw.get("render_pass", L.PBR_SunDepthRenderPass(sp))
    d.vs.glsl_debug_filepath = pbrhip.GPU_String(path, len(path)); d.fs.glsl_debug_filepath = d.vs.glsl_debug_filepath
    fmts = (C.c_int * 4)(pbrhip.Format_RGB32F, pbrhip.Format_RGB32F, pbrhip.Format_RGB32F, pbrhip.Format_RG32F)
    d.vertex_input_formats = C.cast(fmts, C.POINTER(C.c_int)); d.vertex_input_formats_count = 4
    d.enable_depth_test = kw.get("test", True); d.enable_depth_write = kw.get("write", True)
    d.enable_blending = kw.get("blend", False); d.cull_mode = kw.get("cull", pbrhip.CullMode_TwoSided)
    return d, fmts


def test_sun_depth_misuse_reports_once_and_launches_nothing(gpu):
    import pbrhip
    L = gpu
    W = 64
    sp = L.PBR_MakeSunDepthPass(W)
    pos = np.array([[0.5, 0.5, 0.25], [40.5, 0.5, 0.25], [0.5, 40.5, 0.25]], np.float32)
    mesh = pbrhip.make_mesh(pos, np.arange(3, dtype=np.uint32), [(0, 3)])
    M = R.pixel_matrix(W, W)
    g = L.GPU_MakeGraph()
    L.PBR_RecordSunDepthPass(sp, g, mesh, C.byref(_globals(M)))
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    base = _map(L, sp)
    assert base[0, 0] == np.float32(0.25) and base[W - 1, W - 1] == 1.0
    # the reference's pipeline state is accepted through the same path the misuse cases take
    d, keep = _pipeline_desc(L, sp)
    ok = L.GPU_MakeGraphicsPipeline(C.byref(d))
    assert ok
    L.GPU_DestroyGraphicsPipeline(ok)
    tex = pbrhip.make_texture(pbrhip.Format_RGBA16F, W, W, pbrhip.TextureFlag_RenderTarget)
    views = (pbrhip.GPU_TextureView * 1)(pbrhip.GPU_TextureView(tex, 0))
    rd = pbrhip.GPU_RenderPassDesc()
    rd.color_targets_count = 1; rd.color_targets = views; rd.width = W; rd.height = W; rd.depth_stencil_target = L.PBR_SunDepthTexture(sp)
    colour_pass = L.GPU_MakeRenderPass(C.byref(rd))
    with _Errors(L) as msgs:
        for kw in ({"cull": pbrhip.CullMode_DrawCW}, {"cull": pbrhip.CullMode_DrawCCW}, {"blend": True}, {"write": False},
                   {"render_pass": colour_pass}):
            n = len(msgs)
            d, keep = _pipeline_desc(L, sp, **kw)
            assert not L.GPU_MakeGraphicsPipeline(C.byref(d)), kw
            assert len(msgs) == n + 1, (kw, msgs[n:])
        s = L.PBR_SunDepthDescriptorSet(sp)
        # no index buffer bound
        n = len(msgs)
        _record(L, g, sp, mesh, [(s, 3, 1, 0, 0)], clear=False, ib=False)
        assert len(msgs) == n + 1 and "index buffer" in msgs[-1], msgs[n:]
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        # an index range past the buffer
        n = len(msgs)
        _record(L, g, sp, mesh, [(s, 6, 1, 0, 0)], clear=False)
        assert len(msgs) == n + 1 and "outside the bound index buffer" in msgs[-1], msgs[n:]
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        assert np.array_equal(_map(L, sp).view(np.uint32), base.view(np.uint32))
        # a perspective sun matrix fails at submit, before anything of the graph runs (its clear included)
        P = M.copy(); P[3] = np.float32(0.01)
        n = len(msgs)
        L.PBR_RecordSunDepthPass(sp, g, mesh, C.byref(_globals(P)))
        assert len(msgs) == n
        L.GPU_GraphSubmit(g)
        assert len(msgs) == n + 1 and "perspective sun projection not implemented" in msgs[-1], msgs[n:]
        L.GPU_GraphWait(g)
    got = _map(L, sp)
    print(f"misuse: map unchanged in {int((got.view(np.uint32) == base.view(np.uint32)).sum())} of {got.size} texels / tolerance: all")
    assert np.array_equal(got.view(np.uint32), base.view(np.uint32))
    L.GPU_DestroyRenderPass(colour_pass); L.GPU_DestroyTexture(tex)
    L.GPU_DestroyGraph(g); L.PBR_DestroyMesh(mesh); L.PBR_DestroySunDepthPass(sp)
