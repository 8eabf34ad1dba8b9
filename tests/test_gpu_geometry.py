"""K13: the geometry pass (geometry_pass.glsl through GPU_OpDrawIndexed) on the GPU against the CPU reference of the contract
(tests/geometry_raster_ref.py).  Depth, normal, ORM, emissive and velocity are compared bit for bit; base colour
within one 8-bit code (hardware pow).  Every frame is at most 193 x 97 with a few hundred triangles and 32^2 textures."""
import ctypes as C

import numpy as np
import pytest

import geometry_raster_ref as G
import sun_raster_ref as R
from geometry_scenes import crowded_scene, perspective, random_scene, ref_of, tie_grid_scene, two_draw_scene
from gpu_rigs import GeometryRig as Rig

pytestmark = pytest.mark.gpu

f32 = np.float32


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
