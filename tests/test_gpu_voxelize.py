"""K14: the voxelise pass (lightgrid_voxelize.glsl through GPU_OpDraw) on the GPU against the CPU reference of the contract
(tests/voxelize_raster_ref.py): all four fp16 channels of all N^3 voxels and the rejected count, bit for bit.  Bit
identity is what the contract implies: fp64 interpolation from exact integers, the sampler that already makes K13's planes
bit-identical, an EXACT shadow tap, no pow / exp2.  Scenes: tests/voxelize_scenes.py (at most 128^3 and a few hundred triangles; the
end-to-end frame a few thousand)."""
import ctypes as C

import numpy as np
import pytest

import sun_raster_ref as R
import voxelize_raster_ref as V
import voxelize_scenes as S
from gpu_rigs import VoxelizeRig as Rig, voxelize_globals as globals_of

pytestmark = pytest.mark.gpu

f32 = np.float32


def check(name, got, want):
    a, b = np.ascontiguousarray(got).view(np.uint16), np.ascontiguousarray(want).view(np.uint16)
    bad = np.argwhere(a != b)
    print(f"{name}: {len(bad)} differing halfs of {a.size} / tolerance 0 (bit-identical)")
    assert len(bad) == 0, (name, len(bad), bad[:5].tolist())


def run(L, scene):
    import pbrhip
    rig = Rig(L, scene)
    if scene["prior"] is not None:
        pbrhip.upload_mip(rig.tex, 0, np.asarray(scene["prior"], np.float16))
    g = L.GPU_MakeGraph()
    before = L.GPUX_RasterRejectedTriangles()
    rig.record(g)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    got = rig.read()
    rejected = L.GPUX_RasterRejectedTriangles() - before
    L.GPU_DestroyGraph(g)
    rig.destroy()
    return got, rejected


def reaches_cases(scene, infos, rej):
    info = infos[0]
    assert rej == scene["expect"]["rejected"] == 2
    assert (np.bincount(info["axes"][info["axes"] >= 0], minlength=3) > 0).all()              # every dominant axis writes voxels
    assert info["truncated_to_zero"] > 0 and info["contested"] > 0
    last = scene["expect"]["last"]                                                             # the coincident copy in the second draw wins
    assert (info["tri"] == last).sum() > 0 and (info["tri"] == 0).sum() == 0
    assert np.array_equal(info["tris"][last]["uv"], np.zeros((3, 2), f32))                    # and its uv reads fell past the end of SSBO0


def test_voxelize_hand_cases_32(gpu):
    scene, want, infos, rej = S.ref_of("cases", lambda: S.cases_scene(32))
    reaches_cases(scene, infos, rej)
    got, rejected = run(gpu, scene)
    assert rejected == rej
    check("hand cases 32^3", got, want[0])


def reaches_random(scene, want, infos, rej):
    info = infos[0]
    assert rej >= 2 and (np.bincount(info["axes"][info["axes"] >= 0], minlength=3) > 20).all()
    assert info["contested"] > 100 and info["truncated_to_zero"] > 0
    src, dup = scene["dup"]
    assert np.isin(info["tri"], dup).sum() > 0 and np.isin(info["tri"], src).sum() == 0         # duplicates win every voxel of their originals
    a = info["axes"]
    n = len(a)
    for k in range(2 * (n // 20), 3 * (n // 20) - 3, 2):                                        # the face straddlers lose fragments to the range test
        assert (a[k:k + 2] >= 0).any()
    rgb = want[0][..., :3].astype(np.float64)
    own = (info["tri"] >= 0).reshape(rgb.shape[:3])
    assert 0 < (rgb[own].max(1) < 1.0).mean() < 1                                               # dark (shadowed or facing away) and lit voxels both occur


def test_voxelize_random_triangles_128(gpu):
    scene, want, infos, rej = S.ref_of("random", S.random_scene)
    reaches_random(scene, want, infos, rej)
    got, rejected = run(gpu, scene)
    print(f"rejected: GPU {rejected}, reference {rej}")
    assert rejected == rej
    check("random 128^3", got, want[0])


def reaches_load(scene, infos):
    info = infos[0]
    boxes = [(T["box"][2] - T["box"][0] + 1) * (T["box"][3] - T["box"][1] + 1) for T in info["tris"] if T is not None]
    assert sum(b == 64 * 64 for b in boxes) == 3 and sum(b > 64 for b in boxes) >= 3           # the large path: one whole-target box per axis
    assert sorted(info["axes"][:3].tolist()) == [0, 1, 2]
    assert len(info["axes"]) == 602 and scene["passes"][0]["draws"][0]["vertex_count"] % 3 == 2 and len(info["axes"]) % 64 != 0
    cx, cy = scene["column"]
    column = info["hits"].reshape(64, 64, 64)[:, cy, cx]
    assert column.max() > 300 and (column > 100).sum() >= 3                                    # hundreds of triangles on a few keys


def test_voxelize_large_boxes_and_a_contended_column_64(gpu):
    scene, want, infos, rej = S.ref_of("load", S.load_scene)
    reaches_load(scene, infos)
    got, rejected = run(gpu, scene)
    assert rejected == rej == 0
    check("load 64^3", got, want[0])


def test_voxelize_second_pass_without_clear_replay_overlap_and_globals_snapshot(gpu):
    L = gpu
    scene, want, infos, rej = S.ref_of("two", S.two_pass_scene)
    own0, own1 = infos[0]["tri"] >= 0, infos[1]["tri"] >= 0
    assert (own0 & ~own1).sum() > 0 and (own0 & own1).sum() > 0 and (own1 & ~own0).sum() > 0   # kept, overwritten and new voxels
    rig = Rig(L, scene)
    graphs = [L.GPU_MakeGraph(), L.GPU_MakeGraph()]
    try:
        for replay in (0, 1):
            for overlap in (0, 1):
                L.GPUX_SetGraphReplay(replay); L.GPUX_SetGraphOverlap(overlap)
                for f in range(3):                                           # the same graphs submitted again and again
                    g = graphs[f % 2]
                    rig.record(g)
                    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
                    check(f"replay {replay} overlap {overlap} frame {f}", rig.read(), want[1])
        # Globals rewritten between recording and submit: the pass uses what the buffer holds at submit
        g = graphs[0]
        rig.write_globals(globals_of(scene, scale=f32(0.5) * scene["scale"], sun_dir=np.array([1, 0, 0, 0], f32)))
        rig.record(g, write_globals=False)
        rig.write_globals(globals_of(scene))
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        check("Globals rewritten before submit", rig.read(), want[1])
    finally:
        L.GPUX_SetGraphReplay(-1); L.GPUX_SetGraphOverlap(-1)
    for g in graphs:
        L.GPU_DestroyGraph(g)
    rig.destroy()


def test_voxelize_two_grids_in_one_pass_32(gpu):
    """One render-pass instance whose draws name two light grids in turn: d0 -> A, d1 -> B, d1 -> A, d0 -> B.  A draw that names
    another grid than the open job's starts a new job (four K14.cover / K14.resolve), and the jobs run in order: a later job
    overwrites exactly the voxels it owns, so each grid is what one job over its draws in that order leaves."""
    import pbrhip
    L = gpu
    scene = S.cases_scene(32)
    N = scene["N"]
    d0, d1 = S.ref_draws(scene, scene["passes"][0])
    rng = np.random.default_rng(0x5EED1407)
    prior = [rng.uniform(0.0, 4.0, (N, N, N, 4)).astype(np.float16) for _ in range(2)]
    want_a, info = V.voxelize(prior[0], scene["sun_map"], [d0, d1], N)
    want_b, info_b = V.voxelize(prior[1], scene["sun_map"], [d1, d0], N)
    last = scene["expect"]["last"]
    shared = (info["tri"] == last) & (info["hits"] > 1)                      # d1 has one triangle: any other hit is one of d0's
    print(f"two grids 32^3: {int(shared.sum())} voxels of A are owned by d0's job and then by d1's")
    assert shared.sum() > 0 and (info["tri"] >= 0).sum() > shared.sum() and (info_b["tri"] >= 0).sum() > 0
    rig = Rig(L, scene)
    lg_b = L.PBR_MakeLightgrid(N)
    tex = [rig.tex, L.PBR_LightgridTexture(lg_b)]
    for t, p in zip(tex, prior):
        pbrhip.upload_mip(t, 0, p)
    rig.write_globals(globals_of(scene))
    lay, mesh = L.PBR_VoxelizeLayout(rig.vp), rig.meshes[0]

    def make_set(img0, mat):
        s = L.GPU_InitDescriptorSet(None, lay)
        L.GPU_SetBufferBinding(s, 0, L.PBR_VoxelizeGlobalsBuffer(rig.vp))
        L.GPU_SetBufferBinding(s, 1, L.PBR_MeshVertexBuffer(mesh))
        L.GPU_SetBufferBinding(s, 2, L.PBR_MeshIndexBuffer(mesh))
        L.GPU_SetStorageImageBinding(s, 3, img0, 0)
        L.GPU_SetTextureBinding(s, 4, L.PBR_SunDepthTexture(rig.sp))
        L.GPU_SetTextureBinding(s, 5, L.PBR_MaterialTexture(mat, 0))
        L.GPU_SetTextureBinding(s, 6, L.PBR_MaterialTexture(mat, 3))
        L.GPU_SetSamplerBinding(s, 7, L.PBR_VoxelizeShadowSampler(rig.vp))
        L.GPU_SetSamplerBinding(s, 8, L.GPU_SamplerLinearWrap())
        L.GPU_FinalizeDescriptorSet(s)
        return s

    draws = scene["passes"][0]["draws"]
    order = [(0, 0), (1, 1), (1, 0), (0, 1)]                                  # (draw, grid)
    sets = [make_set(tex[t], rig.mats[draws[d]["material"]]) for d, t in order]
    g = L.GPU_MakeGraph()
    L.GPU_OpPrepareRenderPass(g, L.PBR_VoxelizeRenderPass(rig.vp))
    params = [L.GPU_OpPrepareDrawParams(g, L.PBR_VoxelizePipeline(rig.vp), s) for s in sets]
    L.GPU_OpBeginRenderPass(g)
    for p, (d, t) in zip(params, order):
        L.GPU_OpBindDrawParams(g, p)
        L.GPU_OpDraw(g, draws[d]["vertex_count"], draws[d]["instance_count"], draws[d]["first_vertex"], 0)
    L.GPU_OpEndRenderPass(g)
    L.GPUX_EnableOpTiming(1)
    try:
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        names = [L.GPUX_GraphTimedOpName(g, i).decode() for i in range(L.GPUX_GraphTimedOpCount(g))]
    finally:
        L.GPUX_EnableOpTiming(0)
    print(f"two grids 32^3: timed ops {names}")
    assert names.count("K14.cover") == 4 and names.count("K14.resolve") == 4, names
    check("two grids 32^3: grid A = [d0, d1]", pbrhip.read_mip(tex[0], 0), want_a)
    check("two grids 32^3: grid B = [d1, d0]", pbrhip.read_mip(tex[1], 0), want_b)
    L.GPU_DestroyGraph(g)
    for s in sets:
        L.GPU_DestroyDescriptorSet(s)
    L.PBR_DestroyLightgrid(lg_b)
    rig.destroy()


class GPU_SamplerDesc(C.Structure):                                         # include/gpu_hip.h
    _fields_ = [("min_filter", C.c_int), ("mag_filter", C.c_int), ("mipmap_mode", C.c_int), ("address_modes", C.c_int * 3),
                ("mip_lod_bias", C.c_float), ("min_lod", C.c_float), ("max_lod", C.c_float), ("compare_op", C.c_int)]


class _Errors:
    def __init__(self, L):
        self.L, self.msgs = L, []
        self.cb = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)(lambda m, u: self.msgs.append(m.decode()))

    def __enter__(self):
        self.L.GPUX_SetErrorHandler(C.cast(self.cb, C.c_void_p), None)
        return self.msgs

    def __exit__(self, *a):
        self.L.GPUX_SetErrorHandler(None, None)


def test_voxelize_misuse_reports_and_launches_nothing(gpu):
    import pbrhip
    L = gpu
    scene, want, infos, rej = S.ref_of("cases", lambda: S.cases_scene(32))
    N = scene["N"]
    rig = Rig(L, scene)
    g = L.GPU_MakeGraph()
    rig.record(g)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    base = rig.read()
    check("before misuse", base, want[0])
    keep = []

    def make_pass(n=N, color=None, depth=None):
        rd = pbrhip.GPU_RenderPassDesc()
        rd.width = n; rd.height = n
        if color is not None:
            views = (pbrhip.GPU_TextureView * 1)(pbrhip.GPU_TextureView(color, 0))
            keep.append(views)
            rd.color_targets = views; rd.color_targets_count = 1
        if depth is not None:
            rd.depth_stencil_target = depth
        return L.GPU_MakeRenderPass(C.byref(rd))

    def desc(path=b"shaders/lightgrid_voxelize.glsl", **kw):
        d = pbrhip.GPU_GraphicsPipelineDesc()
        d.layout = kw.get("layout", L.PBR_VoxelizeLayout(rig.vp)); d.render_pass = kw.get("render_pass", L.PBR_VoxelizeRenderPass(rig.vp))
        d.vs.glsl_debug_filepath = pbrhip.GPU_String(path, len(path)); d.fs.glsl_debug_filepath = d.vs.glsl_debug_filepath
        if "formats" in kw:
            fm = (C.c_int * len(kw["formats"]))(*kw["formats"])
            keep.append(fm)
            d.vertex_input_formats = C.cast(fm, C.POINTER(C.c_int)); d.vertex_input_formats_count = len(kw["formats"])
        d.enable_conservative_rasterization = kw.get("conservative", True)
        d.enable_depth_test = kw.get("depth_test", False); d.enable_depth_write = kw.get("depth_write", False)
        d.enable_blending = kw.get("blend", False); d.cull_mode = kw.get("cull", pbrhip.CullMode_TwoSided)
        return d

    ok = L.GPU_MakeGraphicsPipeline(C.byref(desc()))
    assert ok
    L.GPU_DestroyGraphicsPipeline(ok)
    colour = pbrhip.make_texture(pbrhip.Format_RGBA8UN, N, N, pbrhip.TextureFlag_RenderTarget)
    sun_tex = L.PBR_SunDepthTexture(rig.sp)
    small = L.GPU_InitPipelineLayout()
    L.GPU_BufferBinding(small, b"GLOBALS")
    L.GPU_FinalizePipelineLayout(small)
    passes = dict(colour=make_pass(color=colour), depth=make_pass(n=scene["sun_map"].shape[0], depth=sun_tex), odd=make_pass(n=36), big=make_pass(n=264))
    with _Errors(L) as msgs:
        # V1: every state the pipeline refuses, one message each
        bad = [({"render_pass": passes["colour"]}, "without colour and depth targets"), ({"render_pass": passes["depth"]}, "without colour and depth targets"),
               ({"render_pass": passes["odd"]}, "multiple of 8"), ({"render_pass": passes["big"]}, "multiple of 8"),
               ({"formats": [pbrhip.Format_RGB32F]}, "no vertex inputs"), ({"conservative": False}, "conservative rasterisation only"),
               ({"cull": pbrhip.CullMode_DrawCCW}, "GPU_CullMode_TwoSided only"), ({"depth_test": True}, "without depth test"),
               ({"depth_write": True}, "without depth test"), ({"blend": True}, "without depth test"), ({"layout": small}, "\"SSBO0\"")]
        for kw, text in bad:
            n = len(msgs)
            assert not L.GPU_MakeGraphicsPipeline(C.byref(desc(**kw))), kw
            assert len(msgs) == n + 1 and text in msgs[-1], (kw, msgs[n:])
        # K12 and K13 keep rejecting conservative rasterisation with their present message
        sun_desc = desc(b"shaders/sun_depth_pass.glsl", render_pass=L.PBR_SunDepthRenderPass(rig.sp), layout=L.PBR_SunDepthLayout(rig.sp),
                        formats=[pbrhip.Format_RGB32F, pbrhip.Format_RGB32F, pbrhip.Format_RGB32F, pbrhip.Format_RG32F], depth_test=True, depth_write=True)
        n = len(msgs)
        assert not L.GPU_MakeGraphicsPipeline(C.byref(sun_desc))
        assert len(msgs) == n + 1 and "blending and conservative rasterisation are not implemented for sun_depth_pass.glsl" in msgs[-1], msgs[n:]
        sun_desc.enable_conservative_rasterization = False
        ok = L.GPU_MakeGraphicsPipeline(C.byref(sun_desc))
        assert ok and len(msgs) == n + 1
        L.GPU_DestroyGraphicsPipeline(ok)
        gb = pbrhip.PBR_GBuffer()
        L.PBR_MakeGBuffer(C.byref(gb), 16, 16, pbrhip.Format_RGBA16F)
        pp = L.PBR_MakePostProcess(C.byref(gb), 16, 16, pbrhip.Format_RGBA8UN)
        gp = L.PBR_MakeGeometryPass(C.byref(gb), pp, 16, 16)
        geo_desc = desc(b"shaders/geometry_pass.glsl", render_pass=L.PBR_GeometryRenderPass(gp, 0), layout=L.PBR_GeometryLayout(gp),
                        formats=[pbrhip.Format_RGB32F, pbrhip.Format_RGB32F, pbrhip.Format_RGB32F, pbrhip.Format_RG32F], depth_test=True, depth_write=True,
                        cull=pbrhip.CullMode_DrawCCW)
        n = len(msgs)
        assert not L.GPU_MakeGraphicsPipeline(C.byref(geo_desc))
        assert len(msgs) == n + 1 and "blending and conservative rasterisation are not implemented for geometry_pass.glsl" in msgs[-1], msgs[n:]
        # V2: every binding the draw checks, by name.  Each set leaves one binding wrong.
        lay, vp = L.PBR_VoxelizeLayout(rig.vp), rig.vp
        mesh, mat = rig.meshes[0], rig.mats[0]
        tiny = L.GPU_MakeBuffer(64, pbrhip.BufferFlag_CPU | pbrhip.BufferFlag_GPU | pbrhip.BufferFlag_StorageBuffer, None)
        grid16 = pbrhip.make_texture(pbrhip.Format_RGBA16F, 16, 16, pbrhip.TextureFlag_StorageImage, depth=16)
        rgba16 = pbrhip.make_texture(pbrhip.Format_RGBA16F, 8, 8, pbrhip.TextureFlag_RenderTarget)
        sd = GPU_SamplerDesc()
        sd.min_filter = sd.mag_filter = sd.mipmap_mode = 0
        for k in range(3):
            sd.address_modes[k] = 1
        sd.max_lod = 1000.0; sd.compare_op = 3                               # LessOrEqual
        wrong_cmp = L.GPU_MakeSampler(C.byref(sd))

        def make_set(**over):
            s = L.GPU_InitDescriptorSet(None, lay)
            L.GPU_SetBufferBinding(s, 0, over.get("globals", L.PBR_VoxelizeGlobalsBuffer(vp)))
            L.GPU_SetBufferBinding(s, 1, over.get("ssbo0", L.PBR_MeshVertexBuffer(mesh)))
            L.GPU_SetBufferBinding(s, 2, over.get("ssbo1", L.PBR_MeshIndexBuffer(mesh)))
            L.GPU_SetStorageImageBinding(s, 3, over.get("img0", rig.tex), 0)
            L.GPU_SetTextureBinding(s, 4, over.get("sun", sun_tex))
            L.GPU_SetTextureBinding(s, 5, over.get("tex0", L.PBR_MaterialTexture(mat, 0)))
            L.GPU_SetTextureBinding(s, 6, over.get("emissive", L.PBR_MaterialTexture(mat, 3)))
            L.GPU_SetSamplerBinding(s, 7, over.get("pcf", L.PBR_VoxelizeShadowSampler(vp)))
            L.GPU_SetSamplerBinding(s, 8, over.get("wrap", L.GPU_SamplerLinearWrap()))
            L.GPU_FinalizeDescriptorSet(s)
            return s

        cases = [(dict(globals=tiny), "GLOBALS", (3, 1, 0, 0)), (dict(ssbo1=tiny), "SSBO1", (18, 1, 0, 0)), (dict(), "SSBO1", (3, 1, len(scene["meshes"][0][1]) - 2, 0)),
                 (dict(img0=grid16), "IMG0", (3, 1, 0, 0)), (dict(sun=rgba16), "SUN_DEPTH_MAP", (3, 1, 0, 0)), (dict(tex0=rgba16), "TEX0", (3, 1, 0, 0)),
                 (dict(emissive=rgba16), "TEX_EMISSIVE", (3, 1, 0, 0)), (dict(wrap=L.GPU_SamplerLinearClamp()), "SAMPLER_LINEAR_WRAP", (3, 1, 0, 0)),
                 (dict(pcf=wrong_cmp), "SAMPLER_PERCENTAGE_CLOSER", (3, 1, 0, 0)), (dict(pcf=L.GPU_SamplerLinearClamp()), "SAMPLER_PERCENTAGE_CLOSER", (3, 1, 0, 0))]
        sets = [make_set(**over) for over, _, _ in cases]
        L.GPU_OpPrepareRenderPass(g, L.PBR_VoxelizeRenderPass(vp))
        params = [L.GPU_OpPrepareDrawParams(g, L.PBR_VoxelizePipeline(vp), s) for s in sets]
        L.GPU_OpBeginRenderPass(g)
        for p, (over, name, draw) in zip(params, cases):
            n = len(msgs)
            L.GPU_OpBindDrawParams(g, p)
            L.GPU_OpDraw(g, *draw)
            assert len(msgs) == n + 1 and "GPU_OpDraw" in msgs[-1] and name in msgs[-1], (name, msgs[n:])
        n = len(msgs)
        L.GPU_OpBindDrawParams(g, params[2])                                 # the good set: an instance count of 0 and less than a triangle draw nothing
        L.GPU_OpDraw(g, 30, 0, 0, 0)
        L.GPU_OpDraw(g, 2, 1, 0, 0)
        L.GPU_OpDrawIndexed(g, 3, 1, 0, 0, 0)                                 # and the pass has no indexed draws
        assert len(msgs) == n + 1 and "GPU_OpDrawIndexed: unsupported (raster)" in msgs[-1], msgs[n:]
        L.GPU_OpEndRenderPass(g)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        # with the lighting pipeline bound GPU_OpDraw behaves as before
        maps = pbrhip.PBR_IBLMaps()
        L.PBR_MakeIBLMaps(C.byref(maps), 16, 64, 32)
        lp = L.PBR_MakeLightingPass(C.byref(gb), C.byref(maps), 16, 16)
        g2 = L.GPU_MakeGraph()
        glob = pbrhip.fill_globals((0.0, -3.0, 1.0), aspect=1.0)
        n = len(msgs)
        L.PBR_RecordLightingPass(lp, g2, C.byref(glob), 0, 0)                # GPU_OpDraw(3, 1, 0, 0): accepted
        assert len(msgs) == n
        L.GPU_OpDraw(g2, 6, 1, 0, 0)
        assert len(msgs) == n + 1 and "only the full-screen triangle GPU_OpDraw(3,1,0,0) of the lighting pass is implemented" in msgs[-1], msgs[n:]
        L.GPU_DestroyGraph(g2)
        L.PBR_DestroyLightingPass(lp); L.PBR_DestroyIBLMaps(C.byref(maps))
    check("after misuse", rig.read(), base)                                  # nothing was launched
    for s in sets:
        L.GPU_DestroyDescriptorSet(s)
    L.GPU_DestroySampler(wrong_cmp); L.GPU_DestroyBuffer(tiny)
    for t in (grid16, rgba16, colour):
        L.GPU_DestroyTexture(t)
    L.PBR_DestroyGeometryPass(gp); L.PBR_DestroyPostProcess(pp); L.PBR_DestroyGBuffer(C.byref(gb))
    for p in passes.values():
        L.GPU_DestroyRenderPass(p)
    L.GPU_DestroyPipelineLayout(small)
    L.GPU_DestroyGraph(g)
    rig.destroy()


def test_voxelize_end_to_end_clear_sun_depth_voxelize_sweeps_128(gpu):
    """One graph: frame-0 clear -> sun depth (K12) -> voxelise (K14) -> three sweeps (K7) over synth_mesh_temple(3000) with four
    materials, through the host layer's PBR_Record* calls, against sun_raster_ref -> the voxelise reference -> the sweep oracle."""
    import pbrhip, pbr_oracle as O
    from pbrhip import synth
    L = gpu
    N, SUN = 128, 256
    verts, idx, parts, part_mat = synth.synth_mesh_temple(3000, n_materials=4)
    mats = synth.synth_materials(4, 32, seed=0x5EED1409)
    materials = [pbrhip.make_material(m) for m in mats]
    mesh = pbrhip.make_mesh(verts, idx, parts)
    for k, m in enumerate(part_mat):
        L.PBR_MeshSetPartMaterial(mesh, k, materials[m])
    lg = L.PBR_MakeLightgrid(N)
    sp = L.PBR_MakeSunDepthPass(SUN)
    vp = pbrhip.make_voxelize_pass(lg, sp)
    glob = pbrhip.fill_globals((0.0, -30.0, 6.0), aspect=16.0 / 9.0)
    g = L.GPU_MakeGraph()
    before = L.GPUX_RasterRejectedTriangles()
    L.PBR_RecordLightgridClear(lg, g)
    L.PBR_RecordSunDepthPass(sp, g, mesh, C.byref(glob))
    L.PBR_RecordVoxelizePass(vp, g, mesh, C.byref(glob))
    tex = L.PBR_LightgridTexture(lg)
    nbytes = L.GPUX_TextureMipBytes(tex, 0)
    bufs = [L.GPU_MakeBuffer(nbytes, pbrhip.BufferFlag_CPU, None) for _ in range(4)]     # the grid after the voxelise pass and after each sweep
    L.GPUX_OpCopyTextureMipToBuffer(g, tex, 0, bufs[0], 0)
    dirs = []
    for k in range(3):
        L.PBR_RecordLightgridSweep(lg, g)
        dirs.append(L.PBR_LightgridSweepDirection(lg))
        L.GPUX_OpCopyTextureMipToBuffer(g, tex, 0, bufs[k + 1], 0)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    rejected = L.GPUX_RasterRejectedTriangles() - before
    got = [np.frombuffer((C.c_char * nbytes).from_address(b.contents.data), np.float16).reshape(N, N, N, 4).copy() for b in bufs]
    # the same chain on the CPU
    sun = np.array(list(glob.sun_space_from_world), f32)
    sun_map, sun_rej = R.raster(np.ones((SUN, SUN), f32), verts[:, :3], idx, [(c, 1, f, 0, sun) for f, c in parts])
    assert np.array_equal(pbrhip.read_mip(L.PBR_SunDepthTexture(sp), 0)[..., 0].view(np.uint32), sun_map.view(np.uint32))
    chains = S.chains(dict(materials=mats))
    flat = np.ascontiguousarray(verts, f32).ravel()
    draws = [dict(vertices=flat, indices=idx, vertex_count=c, instance_count=1, first_vertex=f, scale=f32(glob.lightgrid_scale), sun=sun,
                  sun_dir=np.array(list(glob.sun_direction), f32), material=chains[part_mat[k]]) for k, (f, c) in enumerate(parts)]
    want, info = V.voxelize(np.zeros((N, N, N, 4), np.float16), sun_map, draws, N)
    own = info["tri"] >= 0
    assert own.sum() > 5000 and len(np.unique(info["tri"][own])) > 1000 and (np.bincount(info["axes"][info["axes"] >= 0], minlength=3) > 50).all()
    lit = want[..., :3].astype(np.float64).reshape(-1, 3)[own].max(1)
    assert (lit > 1.0).mean() > 0.05 and (lit < 0.5).mean() > 0.05           # sunlit and shadowed surfaces
    print(f"end to end 128^3: {int(own.sum())} voxels written by {info['fragments']} fragments; rejected GPU {rejected}, reference {sun_rej} + {info['rejected']}")
    assert rejected == sun_rej + info["rejected"]
    check("end to end 128^3: voxelised grid", got[0], want)
    swept = want.view(np.uint16)
    for k, d in enumerate(dirs):
        swept = O.lightgrid_sweep(swept, d)
        check(f"end to end 128^3: after sweep {k} (direction {d})", got[k + 1], swept)
    L.GPU_DestroyGraph(g)
    for b in bufs:
        L.GPU_DestroyBuffer(b)
    L.PBR_DestroyVoxelizePass(vp); L.PBR_DestroyMesh(mesh); L.PBR_DestroySunDepthPass(sp); L.PBR_DestroyLightgrid(lg)
    for m in materials:
        L.PBR_DestroyMaterial(m)
