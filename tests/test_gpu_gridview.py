"""K16, the light-grid visualiser of the lighting pass (Globals.visualize_lightgrid != 0, lighting_pass.glsl:463-491), through the public
path: PBR_MakeLightingPassLive + PBR_RecordLightingPass with the field set.  Every operation of the block is correctly rounded fp32 in
the shader's order and the 3-D sampler is bit-equal between device and oracle, so the RGBA32F target must equal the CPU restatement
(tests/gridview_ref.py) bit for bit on every pixel -- and through it the reference's shader text (tests/golden/gridview_shader_text.npz,
views A and B).  The views are asserted not to be degenerate (misses, late hits, hits on clamped edge voxels from outside the cube)
before anything is compared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gridview_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu


class Rig:
    """IBL maps, the scene's textures and one lighting pass per (size, target format): made once for the module."""

    def __init__(self, L):
        import pbrhip
        from pbrhip import synth
        self.L = L
        self.gbd, grid, levels, sun = V.scene()
        env = synth.synth_env(64, seed=0x5EED00AA)
        self.env_tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 64, 64, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
        self.maps = pbrhip.PBR_IBLMaps()
        L.PBR_MakeIBLMaps(C.byref(self.maps), 16, 64, 32)
        L.PBR_GenIrradianceMap(self.env_tex, self.maps.irradiance_map); L.PBR_GenPrefilteredEnvMap(self.env_tex, self.maps.tex_specular_env_map, 1)
        L.PBR_GenBRDFIntegrationMap(self.maps.brdf_lut)
        n = grid.shape[0]
        self.grid_tex = pbrhip.make_texture(pbrhip.Format_RGBA16F, n, n, pbrhip.TextureFlag_StorageImage, depth=n)
        pbrhip.upload_mip(self.grid_tex, 0, grid)
        self.prev_tex = pbrhip.make_texture(pbrhip.Format_RGBA16F, levels[0].shape[1], levels[0].shape[0], pbrhip.TextureFlag_RenderTarget | pbrhip.TextureFlag_HasMipmaps)
        for m in range(min(self.prev_tex.contents.mip_level_count, len(levels))):
            pbrhip.upload_mip(self.prev_tex, m, levels[m])
        self.sun_tex = pbrhip.make_texture(pbrhip.Format_D32F_Or_X8D24UN, sun.shape[1], sun.shape[0], pbrhip.TextureFlag_RenderTarget)
        pbrhip.upload_mip(self.sun_tex, 0, sun)
        self.flat_tex = pbrhip.make_texture(pbrhip.Format_RGBA16F, 16, 16, pbrhip.TextureFlag_RenderTarget)      # a 2-D texture in the LIGHTGRID slot
        self.passes = {}

    def lighting(self, W, H, fmt, lightgrid="scene"):
        """(G-buffer, lighting pass) of that size and target format; the G-buffer holds the scene at the fixture's size, zeros otherwise
        (the visualiser reads none of it)."""
        import pbrhip
        key = (W, H, fmt, lightgrid)
        if key not in self.passes:
            gb = pbrhip.PBR_GBuffer()
            self.L.PBR_MakeGBuffer(C.byref(gb), W, H, fmt)
            for name, k in (("base_color", "base"), ("normal", "normal"), ("orm", "orm"), ("emissive", "emissive"), ("depth", "depth")):
                a = self.gbd[k]
                pbrhip.upload_mip(getattr(gb, name), 0, a if (W, H) == (V.W, V.H) else np.zeros((H, W) + a.shape[2:], a.dtype))
            grid = {"scene": self.grid_tex, "none": None, "flat": self.flat_tex}[lightgrid]
            lp = self.L.PBR_MakeLightingPassLive(C.byref(gb), C.byref(self.maps), W, H, self.sun_tex, grid, self.prev_tex)
            self.passes[key] = (gb, lp)
        return self.passes[key]

    def close(self):
        L = self.L
        for gb, lp in self.passes.values():
            L.PBR_DestroyLightingPass(lp); L.PBR_DestroyGBuffer(C.byref(gb))
        L.PBR_DestroyIBLMaps(C.byref(self.maps))
        for t in (self.env_tex, self.grid_tex, self.prev_tex, self.sun_tex, self.flat_tex):
            L.GPU_DestroyTexture(t)


@pytest.fixture(scope="module")
def rig(gpu):
    V.check_not_degenerate()
    r = Rig(gpu)
    yield r
    gpu.GPU_WaitUntilIdle()
    r.close()


def globals_of(words, visualize=1):
    import pbrhip
    g = pbrhip.PBR_Globals.from_buffer_copy(np.asarray(words, np.float32).tobytes())
    g.visualize_lightgrid = visualize
    return g


def live_flags():
    import pbrhip
    return pbrhip.Shade_LightShafts | pbrhip.Shade_SunShadows | pbrhip.Shade_VoxelGI


def render(L, gb, lp, glob, flags, bands=((0, 0),), clear=0.25):
    import pbrhip
    L.GPUX_SetShadeFlags(L.PBR_LightingPipeline(lp), flags)
    g = L.GPU_MakeGraph()
    L.GPU_OpClearColorF(g, gb.lighting_result, 0, clear, clear, clear, clear)
    for r0, r1 in bands:
        L.PBR_RecordLightingPass(lp, g, C.byref(glob), r0, r1)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    L.GPU_DestroyGraph(g)
    return pbrhip.read_mip(gb.lighting_result, 0)


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint16)


def describe(got, want):
    """Mismatching pixels of two frames by bits, for an assertion message; the NaN pixels among them are counted."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    bad = (bits(got) != bits(want)).any(-1)
    nan = int(np.isnan(want.astype(np.float32))[bad].any(-1).sum())
    sample = [(yx.tolist(), [hex(v) for v in bits(got)[tuple(yx)]], [hex(v) for v in bits(want)[tuple(yx)]]) for yx in np.argwhere(bad)[:4]]
    return bad, f"{int(bad.sum())} of {bad.size} pixels differ ({nan} of them NaN in the reference); first (pixel, got, want): {sample}"


@pytest.mark.parametrize("view,W,H", [("A", 96, 54), ("B", 96, 54), ("C", 96, 54), ("B", 61, 37)])
def test_gridview_equals_the_restatement_bit_for_bit(gpu, rig, view, W, H):
    import pbrhip
    want, step, _ = V.reference(view, W, H)
    glob = globals_of(V.view_globals(view, W, H))
    print(f"view {view} {W}x{H}: hits {(step >= 0).mean():.3f}, max step {step.max()}, NaN pixels {int(np.isnan(want).any(-1).sum())}")
    gb, lp = rig.lighting(W, H, pbrhip.Format_RGBA32F)
    frames = [render(gpu, gb, lp, glob, flags) for flags in (pbrhip.Shade_IBL, live_flags())]
    for got in frames:
        bad, msg = describe(got, want)
        print("fp32:", msg)
        assert not bad.any(), msg
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))           # the shade flags do not matter in this mode
    if (W, H) == (V.W, V.H) and view in "AB":
        fixture = np.load(V.FIXTURE)["frame_" + view]
        bad, msg = describe(frames[0], fixture)
        assert not bad.any(), "against the reference's shader text: " + msg
    gb16, lp16 = rig.lighting(W, H, pbrhip.Format_RGBA16F)
    got16 = render(gpu, gb16, lp16, glob, pbrhip.Shade_IBL, clear=0.0)                     # RGBA16F targets clear to zero only
    bad, msg = describe(got16, want.astype(np.float16))                                    # numpy converts with round-to-nearest-even
    print("fp16:", msg)
    assert not bad.any(), msg


def test_gridview_row_bands_equal_the_full_frame(gpu, rig):
    import pbrhip
    W, H = V.W, V.H
    glob = globals_of(V.view_globals("B"))
    gb, lp = rig.lighting(W, H, pbrhip.Format_RGBA32F)
    full = render(gpu, gb, lp, glob, live_flags())
    banded = render(gpu, gb, lp, glob, live_flags(), bands=((0, H // 3), (H // 3, H // 2), (H // 2, H)))
    bad, msg = describe(full, V.reference("B")[0])
    assert not bad.any(), msg
    assert np.array_equal(banded.view(np.uint32), full.view(np.uint32))
    one = render(gpu, gb, lp, glob, live_flags(), bands=((H // 3, H // 2),))               # a band alone leaves the other rows cleared
    assert np.array_equal(one[H // 3:H // 2].view(np.uint32), full[H // 3:H // 2].view(np.uint32))
    assert (one[:H // 3] == 0.25).all() and (one[H // 2:] == 0.25).all()


def test_gridview_mode_switch_on_one_graph_with_and_without_replay(gpu, rig):
    """One GPU_Graph runs K5, K16, K16, K5 in four submissions; with hipGraph replay the executable graph built for one kernel must never be
    'updated' into running the other."""
    import pbrhip
    L = gpu
    W, H = V.W, V.H
    words = V.view_globals("B")
    gb, lp = rig.lighting(W, H, pbrhip.Format_RGBA32F)
    shaded = render(L, gb, lp, globals_of(words, 0), live_flags())                         # a plain shaded frame of that pass
    want = V.reference("B")[0]
    assert not np.array_equal(shaded.view(np.uint32), want.view(np.uint32))
    L.GPUX_SetShadeFlags(L.PBR_LightingPipeline(lp), live_flags())
    runs, stats = [], []
    try:
        for replay in (0, 1):
            L.GPUX_SetGraphReplay(replay)
            g = L.GPU_MakeGraph()
            frames = []
            for mode in (0, 1, 1, 0):
                glob = globals_of(words, mode)
                L.GPU_OpClearColorF(g, gb.lighting_result, 0, 0.25, 0.25, 0.25, 0.25)
                L.PBR_RecordLightingPass(lp, g, C.byref(glob), 0, 0)
                L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
                frames.append(pbrhip.read_mip(gb.lighting_result, 0))
            s = [C.c_uint64() for _ in range(3)]
            L.GPUX_GraphReplayStats(g, *[C.byref(v) for v in s])
            stats.append(f"replay {replay}: launches {s[0].value}, updates {s[1].value}, instantiations {s[2].value}")
            L.GPU_DestroyGraph(g)
            runs.append(frames)
    finally:
        L.GPUX_SetGraphReplay(-1)
    print(stats)
    for frames in runs:
        for k, ref in ((0, shaded), (1, want), (2, want), (3, shaded)):
            bad, msg = describe(frames[k], ref)
            assert not bad.any(), (stats, k, msg)
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), stats


@pytest.mark.parametrize("lightgrid", ["none", "flat"])
def test_gridview_without_a_light_grid_is_refused(gpu, rig, lightgrid):
    import pbrhip
    L = gpu
    W, H = V.W, V.H
    gb, lp = rig.lighting(W, H, pbrhip.Format_RGBA32F, lightgrid)
    msgs = []
    CB = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)
    cb = CB(lambda m, u: msgs.append(m.decode()))
    L.GPUX_SetErrorHandler(C.cast(cb, C.c_void_p), None)
    try:
        got = render(L, gb, lp, globals_of(V.view_globals("A")), pbrhip.Shade_IBL)
    finally:
        L.GPUX_SetErrorHandler(None, None)
    assert len(msgs) == 1 and "LIGHTGRID" in msgs[0], msgs
    assert (got == 0.25).all()                                                             # nothing was launched
    shaded = render(L, gb, lp, globals_of(V.view_globals("A"), 0), pbrhip.Shade_IBL)       # mode 0 on the same pass is unaffected
    assert not (shaded == 0.25).all()


def test_channel_split_sampler_equals_the_full_sample_and_the_oracle(gpu):
    """K16 fetches alpha and colour separately (pbrk_debug_sample which = 3): the same bits as K5's grid_sample (which = 0) and as
    orc_tex3d_sample, on the coordinates of test_gpu_parity.py::test_device_samplers_at_wild_coordinates."""
    import pbrhip, pbr_oracle as O
    L = gpu
    rng = np.random.default_rng(0xC00D)
    special = np.array([0.0, -0.0, 1.0, 0.5, 0.25, 1e-30, -1e-30, 1e30, -1e30, np.inf, -np.inf, np.nan, 3.0e9, -3.0e9, 2.0 ** 31, 1.0 - 2.0 ** -24], np.float32)
    coords = np.concatenate([rng.uniform(-0.5, 1.5, (4096, 3)), rng.choice(special, (4096, 3)),
                             np.stack([(np.arange(64) + 0.5) / 64] * 3, -1)]).astype(np.float32)
    n = len(coords)
    cbuf = L.GPU_MakeBuffer(coords.nbytes, pbrhip.BufferFlag_CPU, coords.ctypes.data_as(C.c_void_p))
    obuf = L.GPU_MakeBuffer(n * 16, pbrhip.BufferFlag_CPU, None)
    grid = (rng.random((16, 16, 16, 4)) * 4).astype(np.float16)
    gtex = pbrhip.make_texture(pbrhip.Format_RGBA16F, 16, 16, pbrhip.TextureFlag_StorageImage, depth=16)
    pbrhip.upload_mip(gtex, 0, grid)

    def run(which):
        assert L.pbrk_debug_sample(which, L.GPUX_TextureDevicePtr(gtex, 0), 16, 16, 16, L.GPUX_BufferDevicePtr(cbuf), n, L.GPUX_BufferDevicePtr(obuf), None) == 0
        L.GPU_WaitUntilIdle()
        return np.frombuffer((C.c_char * (n * 16)).from_address(obuf.contents.data), np.float32).reshape(n, 4).copy()

    split, full = run(3), run(0)
    want = np.zeros_like(split)
    g16 = np.ascontiguousarray(grid.view(np.uint16))
    for i in range(n):
        p = np.ascontiguousarray(coords[i])
        O.lib().orc_tex3d_sample(g16.ctypes.data_as(C.c_void_p), 16, p.ctypes.data_as(C.c_void_p), want[i].ctypes.data_as(C.c_void_p))
    assert np.array_equal(split.view(np.uint32), full.view(np.uint32))                     # NaN payloads included: the same device arithmetic
    assert np.array_equal(split, want, equal_nan=True)
    assert np.array_equal(split[:, 3], want[:, 3], equal_nan=True)
    L.GPU_DestroyTexture(gtex); L.GPU_DestroyBuffer(cbuf); L.GPU_DestroyBuffer(obuf)
