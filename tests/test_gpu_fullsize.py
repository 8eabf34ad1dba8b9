"""GPU tests at BASELINE.json's full sizes through size-independent properties (the oracle would need minutes to
hours there): constant environments, linearity, alpha = weight sum, shard = full, plus oracle spot rows; and the
boundary's error behaviour (unknown shader, raster-only calls, incomplete descriptor sets)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REL = 1e-4          # north_star: 1e-4 relative per texel


def _prefilter(gpu, env, spec_size, min_size=1):
    import pbrhip
    W = env.shape[1]
    tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, W, W, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
    spec = pbrhip.make_texture(pbrhip.Format_RGBA32F, spec_size, spec_size,
                               pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps | pbrhip.TextureFlag_StorageImage)
    gpu.PBR_GenPrefilteredEnvMap(tex, spec, min_size)
    return tex, spec


def _host_alpha(gpu, mip):
    rough = [0.0, 0.03, 0.15, 0.4, 0.6][mip] if mip < 5 else min(1.0, float(np.float32(0.6) + np.float32(0.08) * np.float32(mip - 4)))
    tab = np.zeros((8192, 4), np.float32)
    a = C.c_float()
    gpu.pbrk_host_prefilter_table(8192, C.c_float(rough), tab.ctypes.data_as(C.c_void_p), C.byref(a))
    return a.value


def test_c4_constant_environment(gpu):
    """C4 size (4096^2, 13 mips, 2048^2 env): prefilter of a constant environment c is c (mip 0) and c*alpha_mip (MC mips);
    alpha is the host-side weight sum; irradiance 128^2 is c*(N+1)/(2N)."""
    import pbrhip
    c = np.array([0.75, 2.5, 11.0, 1.0], np.float32)
    env = np.empty((6, 2048, 2048, 4), np.float32); env[...] = c
    tex, spec = _prefilter(gpu, env, 4096)
    del env
    for mip in (0, 1, 4, 7, 12):
        got = pbrhip.read_mip(spec, mip)
        if mip == 0:
            assert np.all(got == c)
        else:
            alpha = _host_alpha(gpu, mip)
            assert np.all(got[..., 3] == np.float32(alpha))
            assert np.allclose(got[..., :3], c[:3] * alpha, rtol=3e-5), mip
    irr = pbrhip.make_texture(pbrhip.Format_RGBA32F, 128, 128, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_StorageImage)
    gpu.PBR_GenIrradianceMap(tex, irr)
    got = pbrhip.read_mip(irr, 0)
    assert np.allclose(got[..., :3], c[:3] * (1025.0 / 2048.0), rtol=3e-5) and np.all(got[..., 3] == 0)
    gpu.GPU_DestroyTexture(irr); gpu.GPU_DestroyTexture(spec); gpu.GPU_DestroyTexture(tex)


def test_c2_linearity_and_oracle_rows(gpu, c2_env):
    """C2 size (512^2, 10 mips, 1024^2 env): the filter is linear in the environment; a few rows of every mip match the oracle."""
    import pbrhip, pbr_oracle as O
    env1 = c2_env
    rng = np.random.default_rng(5)
    env2 = np.ascontiguousarray(env1[[1, 0, 3, 2, 5, 4]] * rng.uniform(0.5, 1.5, (6, 1, 1, 4)).astype(np.float32))
    env2[..., 3] = 1.0
    a, b = np.float32(0.25), np.float32(2.0)
    envc = (a * env1 + b * env2).astype(np.float32); envc[..., 3] = 1.0
    outs = []
    for e in (env1, env2, envc):
        tex, spec = _prefilter(gpu, e, 512)
        outs.append([pbrhip.read_mip(spec, m) for m in range(10)])
        gpu.GPU_DestroyTexture(spec); gpu.GPU_DestroyTexture(tex)
    for m in range(10):
        lin = a * outs[0][m][..., :3].astype(np.float64) + b * outs[1][m][..., :3].astype(np.float64)
        got = outs[2][m][..., :3].astype(np.float64)
        err = np.abs(got - lin) / np.maximum(np.abs(lin), 1e-3)
        assert err.max() < 1e-4, (m, err.max())
    pyr = O.build_pyramid(env1)
    for m in (0, 1, 2, 5, 9):
        size = 512 >> m
        for (f, y) in ((0, 0), (2, size // 2), (5, size - 1)):
            want = O.prefilter_mip(pyr, 1024, 512, m, faces=(f, f + 1), rows=(y, y + 1))[f, y]
            err = np.abs(outs[0][m][f, y].astype(np.float64) - want) / np.maximum(np.abs(want), 1e-3)
            assert err.max() < 1e-4, (m, f, y, err.max())


def test_c3_shade_full_frame_properties(gpu):
    """C3 size (1920x1080): banded draws equal the full draw; scaling every emissive byte leaves sky pixels untouched."""
    import pbrhip
    from pbrhip import synth
    W, H = 1920, 1080
    L = gpu
    gbd = synth.synth_gbuffer_spheres(W, H)
    env = synth.synth_env(64, seed=0x5EED00AA)
    env_tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 64, 64, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), 32, 256, 256)
    L.PBR_GenIrradianceMap(env_tex, maps.irradiance_map)
    L.PBR_GenPrefilteredEnvMap(env_tex, maps.tex_specular_env_map, 16)
    L.PBR_GenBRDFIntegrationMap(maps.brdf_lut)
    gb = pbrhip.PBR_GBuffer()
    L.PBR_MakeGBuffer(C.byref(gb), W, H, pbrhip.Format_RGBA16F)
    for name, key in (("base_color", "base"), ("normal", "normal"), ("orm", "orm"), ("emissive", "emissive"), ("depth", "depth")):
        pbrhip.upload_mip(getattr(gb, name), 0, gbd[key])
    lp = L.PBR_MakeLightingPass(C.byref(gb), C.byref(maps), W, H)
    glob = pbrhip.fill_globals(gbd["cam_pos"], aspect=W / H)
    g = L.GPU_MakeGraph()
    L.PBR_RecordLightingPass(lp, g, C.byref(glob), 0, 0)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    full = pbrhip.read_mip(gb.lighting_result, 0).view(np.uint16)
    L.GPU_OpClearColorF(g, gb.lighting_result, 0, 0.0, 0.0, 0.0, 0.0)
    for band in range(8):                                     # the 8-GPU screen split of C5, on one GPU
        L.PBR_RecordLightingPass(lp, g, C.byref(glob), band * 135, (band + 1) * 135)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    banded = pbrhip.read_mip(gb.lighting_result, 0).view(np.uint16)
    assert np.array_equal(full, banded)
    f32 = full.view(np.float16).astype(np.float32)
    # an RGBA16F target saturates to +inf above 65504 (sun highlights): no NaN, no negatives, alpha == 1
    assert not np.isnan(f32).any() and (f32[..., 3] == 1).all() and (f32[..., :3] >= 0).all()
    sky = gbd["depth"] == 1.0
    assert sky.mean() > 0.5 and np.isfinite(f32[sky][:, :3]).mean() > 0.999
    L.GPU_DestroyGraph(g); L.PBR_DestroyLightingPass(lp); L.PBR_DestroyGBuffer(C.byref(gb))
    L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(env_tex)


def test_boundary_error_behaviour(gpu):
    """Reference conventions: shader-compile failure is recoverable (empty string + error array); API misuse and
    raster-only entry points report 'GPU-ERROR' (here through GPUX_SetErrorHandler instead of the default abort)."""
    import pbrhip
    L = gpu
    msgs = []
    CB = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)
    cb = CB(lambda m, u: msgs.append(m.decode()))
    L.GPUX_SetErrorHandler(C.cast(cb, C.c_void_p), None)
    try:
        layout = L.GPU_InitPipelineLayout()
        b_out = L.GPU_StorageImageBinding(layout, b"OUTPUT", pbrhip.Format_RGBA32F)
        b_env = L.GPU_TextureBinding(layout, b"TEX_ENV_CUBE")
        L.GPU_FinalizePipelineLayout(layout)
        desc = pbrhip.GPU_ShaderDesc()
        path = b"../src/demo_pbr_renderer/shaders/taa_resolve.glsl"
        desc.glsl_debug_filepath = pbrhip.GPU_String(path, len(path))
        errs = pbrhip.GPU_GLSLErrorArray()
        tok = L.GPU_SPIRVFromGLSL(None, 2, layout, C.byref(desc), C.byref(errs))
        assert tok.length == 0 and errs.length == 1 and b"no built-in kernel" in errs.data[0].error_message.data
        joined = L.GPU_JoinGLSLErrorString(None, errs)
        assert joined.length > 0 and not msgs
        # a known shader compiles to an opaque token and makes a pipeline
        path2 = b"C:/x/shaders\\gen_prefiltered_env_map.glsl"
        desc2 = pbrhip.GPU_ShaderDesc(); desc2.glsl_debug_filepath = pbrhip.GPU_String(path2, len(path2))
        tok2 = L.GPU_SPIRVFromGLSL(None, 2, layout, C.byref(desc2), C.byref(errs))
        assert tok2.length > 0 and errs.length == 0
        desc2.spirv = tok2
        pipe = L.GPU_MakeComputePipeline(layout, C.byref(desc2))
        assert pipe
        # descriptor set with a missing binding: Finalize reports (gpu_vulkan.c:841,849)
        ds = L.GPU_InitDescriptorSet(None, layout)
        out = pbrhip.make_texture(pbrhip.Format_RGBA32F, 32, 32, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_StorageImage | pbrhip.TextureFlag_HasMipmaps)
        L.GPU_SetStorageImageBinding(ds, b_out, out, 0)
        L.GPU_FinalizeDescriptorSet(ds)
        assert msgs and "never set" in msgs[-1]
        # binding a texture without the StorageImage flag as a storage image
        plain = pbrhip.make_texture(pbrhip.Format_RGBA32F, 32, 32, pbrhip.TextureFlag_Cubemap)
        n = len(msgs); L.GPU_SetStorageImageBinding(ds, b_out, plain, 0); assert len(msgs) == n + 1
        # storage binding beyond the mip chain
        n = len(msgs); L.GPU_SetStorageImageBinding(ds, b_out, out, 99); assert len(msgs) == n + 1
        # raster-only entry points
        g = L.GPU_MakeGraph()
        n = len(msgs); L.GPU_OpDrawIndexed(g, 3, 1, 0, 0, 0); assert len(msgs) == n + 1 and "unsupported (raster)" in msgs[-1]
        n = len(msgs); L.GPU_OpDraw(g, 6, 1, 0, 0); assert len(msgs) == n + 1
        # dispatch without a bound set; dispatch with zero groups
        L.GPU_OpBindComputePipeline(g, pipe)
        n = len(msgs); L.GPU_OpDispatch(g, 4, 4, 1); assert len(msgs) == n + 1
        n = len(msgs); L.GPU_OpDispatch(g, 0, 4, 1); assert len(msgs) == n + 1
        # zero-extent texture (gpu_vulkan.c:1339) and zero-size buffer
        n = len(msgs); assert not L.GPU_MakeTexture(pbrhip.Format_RGBA32F, 0, 4, 1, 0, None); assert len(msgs) == n + 1
        # an empty graph submits and waits fine; NULL destroys are accepted where the reference documents them
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        L.GPU_DestroyTexture(None); L.GPU_DestroyBuffer(None); L.GPU_DestroyComputePipeline(None); L.GPU_DestroyDescriptorSet(None)
        L.GPU_DestroyDescriptorArena(None); L.GPU_DestroyGraphicsPipeline(None)
        L.GPU_DestroyGraph(g); L.GPU_DestroyDescriptorSet(ds); L.GPU_DestroyComputePipeline(pipe)
        L.GPU_DestroyTexture(out); L.GPU_DestroyTexture(plain); L.GPU_DestroyPipelineLayout(layout)
    finally:
        L.GPUX_SetErrorHandler(None, None)


def test_c_demo_hdr_file_end_to_end(gpu, tmp_path):
    """The plain-C driver (host/pbr_demo.c: GPU_Init -> .hdr strip file -> IBL precompute -> lighting pass) agrees with the
    same sequence driven from Python through ctypes: file decode (RLE .hdr), mip chain, all maps, lit frame."""
    import os, subprocess
    import pbrhip
    from pbrhip import synth
    env = synth.synth_env(64, seed=0x5EED00AA)
    hdr = tmp_path / "cube_strip.hdr"
    hdr.write_bytes(synth.env_to_hdr_strip(env, rle=True))
    exe = os.path.join(pbrhip.PKG_ROOT, "pbr_demo")
    ppm = tmp_path / "frame.ppm"
    out = subprocess.run([exe, str(hdr), "32", "256", "64", "16", "320", "180", str(ppm)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    kv = {}
    for line in out.stdout.splitlines():
        parts = line.split()
        if parts[0] != "time_ms":
            kv[parts[0]] = float(parts[1])
    assert kv["ok"] == 1 and kv["env_size"] == 64 and kv["env_mips"] == 7
    # Python path on the same data (the RGBE round trip of synth_env makes the decoded file equal to `env`)
    L = gpu
    tex = L.PBR_MakeTextureFromHDRIFile(str(hdr).encode())
    assert tex and tex.contents.width == 64
    assert np.array_equal(pbrhip.read_mip(tex, 0), env)
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), 32, 256, 64)
    L.PBR_GenIrradianceMap(tex, maps.irradiance_map)
    L.PBR_GenPrefilteredEnvMap(tex, maps.tex_specular_env_map, 16)
    L.PBR_GenBRDFIntegrationMap(maps.brdf_lut)

    def fsum(a):
        return float(a.astype(np.float64).sum())
    assert kv["env_mip0_sum"] == pytest.approx(fsum(pbrhip.read_mip(tex, 0)), rel=1e-9)
    assert kv["env_last_mip_sum"] == pytest.approx(fsum(pbrhip.read_mip(tex, 6)), rel=1e-9)
    assert kv["irradiance_sum"] == pytest.approx(fsum(pbrhip.read_mip(maps.irradiance_map, 0)), rel=1e-9)
    for m in range(3):
        assert kv[f"specular_mip{m}_sum"] == pytest.approx(fsum(pbrhip.read_mip(maps.tex_specular_env_map, m)), rel=1e-9)
    assert "specular_mip3_sum" not in kv                      # reference stop rule: size < 16 (render.cpp:566)
    assert kv["lut_bits_sum"] == fsum(pbrhip.read_mip(maps.brdf_lut, 0).view(np.uint16))
    assert kv["lit_bits_sum"] > 0

    # the per-frame chain of the demo (lighting -> TAA -> bloom -> tone map, three frames) and its light-grid sweeps, from Python
    W, H = 320, 180
    gb = pbrhip.PBR_GBuffer()
    L.PBR_MakeGBuffer(C.byref(gb), W, H, pbrhip.Format_RGBA16F)
    plane = lambda rgba: np.broadcast_to(np.array(rgba, np.uint8), (H, W, 4)).copy()
    pbrhip.upload_mip(gb.base_color, 0, plane((255, 195, 86, 255))); pbrhip.upload_mip(gb.normal, 0, plane((128, 128, 255, 255)))
    pbrhip.upload_mip(gb.orm, 0, plane((255, 90, 255, 255))); pbrhip.upload_mip(gb.emissive, 0, plane((0, 0, 0, 255)))
    depth = np.ones((H, W), np.float32); depth[H // 2:] = 0.998
    pbrhip.upload_mip(gb.depth, 0, depth)
    lp = L.PBR_MakeLightingPass(C.byref(gb), C.byref(maps), W, H)
    pp = L.PBR_MakePostProcess(C.byref(gb), W, H, pbrhip.Format_RGBA8UN)
    g = L.GPU_MakeGraph()
    glob = pbrhip.fill_globals((0.0, 0.0, 5.0), aspect=W / H, frame_idx=0)
    L.PBR_RecordLightingPass(lp, g, C.byref(glob), 0, 0)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    assert kv["lit_bits_sum"] == fsum(pbrhip.read_mip(gb.lighting_result, 0).view(np.uint16))
    for frame in range(3):
        glob = pbrhip.fill_globals((0.0, 0.0, 5.0), aspect=W / H, frame_idx=frame)
        L.PBR_RecordLightingPass(lp, g, C.byref(glob), 0, 0)
        L.PBR_RecordTaaResolve(pp, g, frame); L.PBR_RecordBloom(pp, g, frame); L.PBR_RecordFinalPostProcessBloom(pp, g, frame)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    L.GPU_DestroyGraph(g)
    assert kv["taa_bits_sum"] == fsum(pbrhip.read_mip(L.PBR_PostTaaOutput(pp, 0), 0).view(np.uint16))
    assert kv["bloom_bits_sum"] == fsum(pbrhip.read_mip(L.PBR_PostBloomUpscale(pp), 0).view(np.uint16))
    bb = pbrhip.read_mip(L.PBR_PostBackbuffer(pp), 0)
    assert kv["frame_bytes_sum"] == fsum(bb)
    raw = ppm.read_bytes()
    head = b"P6\n320 180\n255\n"
    assert raw.startswith(head) and len(raw) == len(head) + W * H * 3
    assert np.array_equal(np.frombuffer(raw[len(head):], np.uint8).reshape(H, W, 3), bb[..., :3])
    assert bb[: H // 2, :, :3].mean() > 30 and bb[H // 2:, :, :3].mean() > 10           # a visible sky and a lit floor
    lg = L.PBR_MakeLightgrid(128)
    scene = np.zeros((128, 128, 128, 4), np.uint16)
    scene[:4] = [0x3800, 0x3400, 0x3000, 0x3C00]
    g = L.GPU_MakeGraph()
    L.PBR_RecordLightgridClear(lg, g)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    pbrhip.upload_mip(L.PBR_LightgridTexture(lg), 0, scene)
    for _ in range(3):
        L.PBR_RecordLightgridSweep(lg, g)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g); L.GPU_DestroyGraph(g)
    assert kv["lightgrid_bits_sum"] == fsum(pbrhip.read_mip(L.PBR_LightgridTexture(lg), 0).view(np.uint16))
    L.PBR_DestroyLightgrid(lg); L.PBR_DestroyPostProcess(pp); L.PBR_DestroyLightingPass(lp); L.PBR_DestroyGBuffer(C.byref(gb))
    L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(tex)


def test_equirect_to_cube_and_hdr_writer(gpu, tmp_path):
    """Extension: K6 equirect -> cube vs the oracle, and the RGBE writer round trip through the strip loader."""
    import pbrhip, pbr_oracle as O
    from pbrhip import synth
    rng = np.random.default_rng(0x5EED00AF)
    h, w = 96, 192
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    pano = np.ones((h, w, 4), np.float32)
    pano[..., 0] = 0.5 + 0.4 * np.sin(xx * 2 * np.pi / w * 3)
    pano[..., 1] = 0.2 + yy / h
    pano[..., 2] = rng.random((h, w)).astype(np.float32)
    pano[20:22, 50:52, :3] = 5.0e4                                   # an HDR "sun"
    tex = gpu.GPUX_MakeCubemapFromEquirect(pano.ctypes.data_as(C.c_void_p), w, h, 64, 0)
    assert tex and tex.contents.mip_level_count == 7 and tex.contents.layer_count == 6
    got = pbrhip.read_mip(tex, 0)
    want = O.equirect_to_cube(pano, 64)
    err = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-3)
    assert err.max() < 1e-4, err.max()
    assert (got.view(np.uint32) == want.view(np.uint32)).mean() > 0.6
    # the mip chain was generated from the converted level
    pyr = O.build_pyramid(got)
    assert np.array_equal(pbrhip.read_mip(tex, 3), O.pyramid_level(pyr, 64, 3))
    # a constant panorama converts to a constant cube
    const = np.empty((8, 16, 4), np.float32); const[...] = (3.0, 0.25, 7.0, 1.0)
    t2 = gpu.GPUX_MakeCubemapFromEquirect(const.ctypes.data_as(C.c_void_p), 16, 8, 16, 0)
    assert np.all(pbrhip.read_mip(t2, 0) == const[0, 0])
    # RGBE writer: cube strip written by the library is read back by the reference-path loader
    env = synth.synth_env(16, seed=0x5EED00AD)
    t3 = pbrhip.make_texture(pbrhip.Format_RGBA32F, 16, 16, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
    path = str(tmp_path / "strip.hdr").encode()
    assert gpu.PBR_WriteCubeStripHDR(path, t3, 0) == 0
    t4 = gpu.PBR_MakeTextureFromHDRIFile(path)
    assert t4 and np.array_equal(pbrhip.read_mip(t4, 0), env)           # env is RGBE-representable: lossless round trip
    # and the oracle's decoder reads the same file identically
    assert np.array_equal(O.rgbe_decode(open(path, "rb").read()).reshape(6, 16, 16, 4), env)
    for t in (tex, t2, t3, t4):
        gpu.GPU_DestroyTexture(t)


def test_bench_accepts_real_files_by_path(gpu, tmp_path):
    """VERDICT r2 item 8 / SURVEY 7 item 7: `bench.py --hdr FILE` (a Radiance cube strip through PBR_MakeTextureFromHDRIFile, here with
    96^2 faces -- not a power of two -- or a 2:1 panorama through the equirect loader) and `--gbuffer DIR` (the five planes as .npy)
    replace the synthetic inputs; the JSON line says data = "file" and carries the SHA-256 of what was read; --check still holds."""
    import hashlib, json, os, subprocess, sys
    import pbrhip
    from pbrhip import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = synth.synth_env(96, seed=0x5EED00B9)
    strip = tmp_path / "strip96.hdr"
    strip.write_bytes(synth.env_to_hdr_strip(env, rle=True))
    yy, xx = np.mgrid[0:128, 0:256]
    pano = np.zeros((128, 256, 4), np.float32)
    pano[..., 0] = 0.2 + xx / 256.0; pano[..., 1] = 0.3 + yy / 128.0; pano[..., 2] = 0.5; pano[60:64, 100:104, :3] = 900.0; pano[..., 3] = 1.0
    eq = tmp_path / "pano.hdr"
    assert gpu.PBR_WriteHDRFile(str(eq).encode(), pano.ctypes.data_as(C.c_void_p), 256, 128) == 0
    gdir = tmp_path / "gbuffer"; gdir.mkdir()
    gbd = synth.synth_gbuffer_spheres(320, 180)
    for name, key in (("base_color", "base"), ("normal", "normal"), ("orm", "orm"), ("emissive", "emissive"), ("depth", "depth")):
        np.save(gdir / (name + ".npy"), gbd[key])
    (gdir / "camera.json").write_text(json.dumps({"pos": [float(v) for v in gbd["cam_pos"]], "fov": 75.0}))
    env_vars = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    for hdr, layout, cube in ((strip, "cube strip", 96), (eq, "equirectangular", 256)):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--workload", "ref", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-c5",
                            "--check", "--hdr", str(hdr), "--gbuffer", str(gdir)], capture_output=True, text=True, timeout=900, env=env_vars, cwd=root)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert out["data"] == "file"
        assert out["inputs"]["hdr"]["layout"] == layout and out["inputs"]["hdr"]["sha256"] == hashlib.sha256(hdr.read_bytes()).hexdigest()
        assert f"cube {cube}^2" in out["config"]["workload"] and out["inputs"]["hdr"]["sha256"] in out["config"]["env"]
        assert out["inputs"]["gbuffer"]["width"] == 320 and out["extra"]["shade"]["mpixels_per_s_kernel"] > 0, out["extra"].get("shade_error")
        assert "320x180" in out["extra"]["shade"]["workload"]
        assert out["extra"]["check_max_rel_err_vs_oracle"] < 1e-4


def test_bench_plain_run_dumps_the_maps_of_its_last_step(gpu, tmp_path):
    """A plain `bench.py` run (no --full) times its steps and prints the headline without the per-kernel, extra and CPU-baseline
    legs; `--dump-outputs DIR` writes the maps of the last timed step as float32 .npy files (64 MB at most), which match the oracle
    on spot rows of the same seeded environment."""
    import json, os, subprocess, sys
    import pbr_oracle as O
    from pbrhip import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dump = tmp_path / "dump"
    env_vars = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "ref", "--steps", "2", "--warmup", "1", "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=900, env=env_vars, cwd=root)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "Mtexels/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["full"] is False
    assert out["kernels"] is None and out["roofline"] is None and out["cpu_baseline"] is None and "shade" not in out["extra"]
    files = {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}
    assert set(files) == {"irradiance"} | {f"specular_mip{m}" for m in range(9)}
    assert all(a.dtype == np.float32 for a in files.values()) and sum(a.nbytes for a in files.values()) <= 64 << 20
    pyr = O.build_pyramid(synth.synth_env(256, seed=0x5EED00AB))            # the `ref` workload's environment
    for m in (0, 1, 2, 4):
        size = 256 >> m
        got = files[f"specular_mip{m}"]
        assert got.shape == (6, size, size, 4)
        for (f, y) in ((0, 0), (3, size // 2), (5, size - 1)):
            want = O.prefilter_mip(pyr, 256, 256, m, faces=(f, f + 1), rows=(y, y + 1))[f, y]
            err = np.abs(got[f, y].astype(np.float64) - want) / np.maximum(np.abs(want), 1e-3)
            assert err.max() < REL, (m, f, y, err.max())
    want = O.irradiance(pyr, 256, 32, faces=(2, 3), rows=(5, 6))[2, 5, :, :3]
    got = files["irradiance"][2, 5, :, :3].astype(np.float64)
    assert (np.abs(got - want) / np.maximum(np.abs(want), 1e-3)).max() < REL


def test_soak_random_environments_and_rows(gpu):
    """the soak of tools/soak_ibl.py as a (bounded) test.  Four random HDR environments (seeded: size, output size, sun
    direction at 5e4:1 contrast) through the whole precompute -- every texel of every mip and the irradiance map vs the oracle at 1e-4,
    mip chain bit for bit -- then two environments at sizes the region kernel serves (256 -> 512, 512 -> 1024): three random
    (face, row) pairs of every level >= 256^2 vs the oracle.  The region kernel's completeness counter must stay at zero."""
    import pbrhip, pbr_oracle as O
    from pbrhip import mc, synth
    L = gpu
    rng = np.random.default_rng(0x50AC)
    sun0 = synth.SUN_DIR.copy()

    def rel(a, b, floor=1e-3):
        return float((np.abs(a.astype(np.float64) - b) / np.maximum(np.abs(b), floor)).max())
    try:
        for run in range(4):
            W = int(rng.choice([32, 64, 128])); out = int(rng.choice([16, 32, 64]))
            d = rng.normal(size=3); synth.SUN_DIR = d / np.linalg.norm(d)
            env = synth.synth_env(W, seed=int(rng.integers(1, 2 ** 31)), workers=1)
            pyr = O.build_pyramid(env)
            tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, W, W, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
            maps = pbrhip.PBR_IBLMaps()
            L.PBR_MakeIBLMaps(C.byref(maps), 16, 64, out)
            L.PBR_GenPrefilteredEnvMap(tex, maps.tex_specular_env_map, 1)
            L.PBR_GenIrradianceMap(tex, maps.irradiance_map)
            for m in range(maps.tex_specular_env_map.contents.mip_level_count):
                e = rel(pbrhip.read_mip(maps.tex_specular_env_map, m), O.prefilter_mip(pyr, W, out, m))
                assert e < REL, (run, W, out, m, e)
            assert rel(pbrhip.read_mip(maps.irradiance_map, 0)[..., :3], O.irradiance(pyr, W, 16)[..., :3]) < REL, (run, W)
            for l in range(tex.contents.mip_level_count):
                assert np.array_equal(pbrhip.read_mip(tex, l), O.pyramid_level(pyr, W, l)), (run, l)
            L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(tex)
        for (W, out) in ((256, 512), (512, 1024)):
            d = rng.normal(size=3); synth.SUN_DIR = d / np.linalg.norm(d)
            env = synth.synth_env(W, seed=int(rng.integers(1, 2 ** 31)), workers=1)
            pyr = O.build_pyramid(env)
            tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, W, W, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
            maps = pbrhip.PBR_IBLMaps()
            L.PBR_MakeIBLMaps(C.byref(maps), 16, 64, out)
            L.PBR_GenPrefilteredEnvMap(tex, maps.tex_specular_env_map, 256)
            for m in range(maps.tex_specular_env_map.contents.mip_level_count):
                size = out >> m
                if size < 256:
                    break
                got = pbrhip.read_mip(maps.tex_specular_env_map, m)
                for _ in range(3):
                    f, y = int(rng.integers(0, 6)), int(rng.integers(0, size))
                    want = O.prefilter_mip(pyr, W, out, m, faces=(f, f + 1), rows=(y, y + 1))[f, y]
                    assert rel(got[f, y], want) < REL, (W, out, m, f, y)
            L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(tex)
    finally:
        synth.SUN_DIR = sun0
    st = mc.counters(L, "region", missing_ok=True)
    if st:
        assert st["healed"] == 0, f"{st['healed']} of {st['slices']} wave-slices had to be recomputed"
