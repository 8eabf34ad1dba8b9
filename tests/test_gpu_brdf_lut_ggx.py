"""K22 on the GPU: the GGX split-sum BRDF LUT (GPUX_OpBrdfLutGGX, csrc/k_lut_ggx.hip) against the numpy restatement of
tests/brdf_lut_ggx_ref.py, through the graph op, row ranges, the three target formats, hipGraph replay, the host layer, the lighting
pass and pbr_demo.

Criterion of every value comparison: the reference of a texel is the fp64 sum of the restatement's N per-sample fp32 terms, divided by
N.  The terms are bit-identical by contract and non-negative, so any fp32 accumulation order (fused or not) errs by at most
(N + 2) 2^-24 relative to first order: asserted is |gpu - ref| <= (N + 2) 2^-23 ref + N 2^-126, the second summand for terms in the
subnormal range, whichever way the device treats them.  Values are compared on RG32F targets.

The kernel has one code path per visibility term; what switches is the number of waves S that share a group of 64 columns
(blg_slices of csrc/brdf_lut_ggx_core.h): 16 up to 64 columns, 8 up to 128, 4 up to 256, 2 up to 512, and 1 above, where a wave walks
groups wave, wave + 16, ..."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import brdf_lut_ggx_ref as B  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-3.0)
VIS = [B.SCHLICK, B.CORRELATED]
_REF = {}


def reference(w, h, count, vis):
    """float64 [h][w][2], computed once per (w, h, N, term) and shared, never written"""
    import pbrhip
    key = (w, h, count, vis)
    if key not in _REF:
        _REF[key] = B.lut_f64(w, h, pbrhip.brdf_lut_ggx_samples(count), vis)
        _REF[key].setflags(write=False)
    return _REF[key]


def target(fmt, w, h):
    """a 2-D texture whose every texel holds the sentinel"""
    import pbrhip
    tex = pbrhip.make_texture(fmt, w, h, pbrhip.TextureFlag_StorageImage)
    dt, ch = pbrhip._FMT_NP[fmt]
    pbrhip.upload_mip(tex, 0, np.full((h, w, ch), SENTINEL, dt))
    return tex


def bake(w, h, count, vis, fmt=None, rows=None):
    """the map as numpy after one op on a sentinel-filled target"""
    import pbrhip
    tex = target(pbrhip.Format_RG32F if fmt is None else fmt, w, h)
    try:
        pbrhip.brdf_lut_ggx(tex, count, vis, rows)
        return pbrhip.read_mip(tex, 0)
    finally:
        pbrhip.lib().GPU_DestroyTexture(tex)


def check(label, got, want, count):
    g = got.astype(np.float64)
    bound = (count + 2) * 2.0 ** -23 * want + count * 2.0 ** -126
    err = np.abs(g - want)
    assert np.isfinite(g).all(), label
    bad = err > bound
    assert not bad.any(), (label, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float((err / np.maximum(want, 1e-300)).max()))


# w x h: what each can break
SHAPES = [(1, 1),        # one lane of one wave; 15 waves hold a share each
          (5, 3),        # a few lanes, rectangular indexing
          (37, 37),      # ragged against 64 lanes
          (64, 64),      # one full group of columns
          (65, 64)]      # two groups, the second with one live lane; 8 waves per group


@pytest.mark.parametrize("vis", VIS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_map_is_within_the_accumulation_bound(gpu, w, h, vis):
    for count in (1, 16, 64):                                                  # N = 1: fifteen of sixteen waves have no sample
        check(f"{w} x {h} N {count} term {vis}", bake(w, h, count, vis), reference(w, h, count, vis), count)


@pytest.mark.parametrize("vis", VIS)
@pytest.mark.parametrize("count", [63, 65, 1024, 4096])
def test_sample_counts_at_the_run_edges_and_the_cap(gpu, count, vis):
    """16 x 16, 16 runs: 63 -> runs of 4 with a last run of 3, 65 -> runs of 5 with two empty runs, 4096 -> the whole 64 KB table"""
    check(f"16 x 16 N {count} term {vis}", bake(16, 16, count, vis), reference(16, 16, count, vis), count)


@pytest.mark.parametrize("vis", VIS)
def test_full_size_map(gpu, vis):
    """256 x 256 at N = 64: 256 workgroups, four groups of columns with four waves each; row 0 (r = 1/512) and column 0 (N.V = 1/512)"""
    got = bake(256, 256, 64, vis)
    check(f"256 x 256 term {vis}", got, reference(256, 256, 64, vis), 64)
    assert (got >= 0).all()


@pytest.mark.parametrize("w,h", [(320, 2), (577, 2), (1030, 1)])
def test_wide_maps_take_the_other_splits(gpu, w, h):
    """320 columns: 5 groups, 2 waves each; 577: 10 groups, one wave each, six waves idle; 1030: 17 groups, wave 0 walks two of them"""
    for count, vis in ((16, B.SCHLICK), (65, B.CORRELATED)):
        check(f"{w} x {h} N {count} term {vis}", bake(w, h, count, vis), reference(w, h, count, vis), count)


# ---- row ranges ----
@pytest.mark.parametrize("vis", VIS)
def test_row_ranges_write_the_same_bytes_and_nothing_else(gpu, vis):
    import pbrhip
    w = h = 37
    whole = bake(w, h, 64, vis)
    assert (whole != SENTINEL).all()
    part = bake(w, h, 64, vis, rows=(3, 11))
    inside = np.zeros((h, w), bool)
    inside[3:11] = True
    assert (part[~inside] == SENTINEL).all()
    assert part[inside].tobytes() == whole[inside].tobytes()
    halves = target(pbrhip.Format_RG32F, w, h)
    try:
        pbrhip.brdf_lut_ggx(halves, 64, vis, (0, 18))
        pbrhip.brdf_lut_ggx(halves, 64, vis, (18, h))
        assert pbrhip.read_mip(halves, 0).tobytes() == whole.tobytes()
    finally:
        gpu.GPU_DestroyTexture(halves)


# ---- formats ----
@pytest.mark.parametrize("vis", VIS)
@pytest.mark.parametrize("w,h", [(37, 37), (65, 64)])
def test_other_formats_hold_the_same_values(gpu, w, h, vis):
    """RG16F: the round-to-nearest-even conversion of the RG32F result (numpy's astype); RGBA32F: (A, B, 0, 1)"""
    import pbrhip
    f32 = bake(w, h, 64, vis)
    f16 = bake(w, h, 64, vis, fmt=pbrhip.Format_RG16F)
    assert f16.dtype == np.float16 and f16.tobytes() == f32.astype(np.float16).tobytes()
    f4 = bake(w, h, 64, vis, fmt=pbrhip.Format_RGBA32F)
    want = np.concatenate([f32, np.zeros((h, w, 1), np.float32), np.ones((h, w, 1), np.float32)], -1)
    assert f4.tobytes() == want.tobytes()


# ---- repeatability, replay ----
def test_the_same_op_twice_gives_the_same_bytes(gpu):
    for w, h in ((16, 16), (256, 8), (577, 2)):
        assert bake(w, h, 64, B.SCHLICK).tobytes() == bake(w, h, 64, B.SCHLICK).tobytes()


def test_graph_replay_captures_the_op(gpu):
    """nothing is allocated when the op executes, so a graph holding it is captured and replayed; the bytes are the plain submit's"""
    import pbrhip
    L = gpu
    want = bake(37, 37, 64, B.CORRELATED)
    dst = target(pbrhip.Format_RG32F, 37, 37)
    g = L.GPU_MakeGraph()
    try:
        L.GPUX_SetGraphReplay(1)
        for _ in range(2):
            pbrhip.upload_mip(dst, 0, np.full((37, 37, 2), SENTINEL, np.float32))
            L.GPUX_OpBrdfLutGGX(g, dst, 64, B.CORRELATED, 0, 37)
            L.GPU_GraphSubmit(g)
            L.GPU_GraphWait(g)
            assert pbrhip.read_mip(dst, 0).tobytes() == want.tobytes()
        s = [C.c_uint64(0) for _ in range(3)]
        L.GPUX_GraphReplayStats(g, *[C.byref(v) for v in s])
        assert s[0].value == 2 and s[1].value + s[2].value == 2, [v.value for v in s]
    finally:
        L.GPUX_SetGraphReplay(-1)
        L.GPU_DestroyGraph(g)
        L.GPU_DestroyTexture(dst)


# ---- argument checks ----
def test_bad_arguments_are_one_error_each_and_record_nothing(gpu):
    import pbrhip
    L = gpu
    messages = []
    handler = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)(lambda msg, user: messages.append(msg.decode()))
    dst = target(pbrhip.Format_RG32F, 8, 8)
    half4 = pbrhip.make_texture(pbrhip.Format_RGBA16F, 8, 8, pbrhip.TextureFlag_StorageImage)
    cube = pbrhip.make_texture(pbrhip.Format_RGBA32F, 8, 8, pbrhip.TextureFlag_StorageImage | pbrhip.TextureFlag_Cubemap)
    vol = pbrhip.make_texture(pbrhip.Format_RGBA32F, 8, 8, pbrhip.TextureFlag_StorageImage, depth=4)
    wide = pbrhip.make_texture(pbrhip.Format_RG16F, 4097, 1, pbrhip.TextureFlag_StorageImage)
    sun = L.PBR_MakeSunDepthPass(64)
    g = L.GPU_MakeGraph()
    L.GPUX_SetErrorHandler(C.cast(handler, C.c_void_p), None)
    L.GPUX_EnableOpTiming(1)
    try:
        bad = [(None, 16, 0, 0, 8),                                            # NULL
               (half4, 16, 0, 0, 8), (cube, 16, 0, 0, 8), (vol, 16, 0, 0, 8),    # a format, a cube, a 3-D texture
               (wide, 16, 0, 0, 1),                                            # above 4096 a side
               (dst, 0, 0, 0, 8), (dst, 4097, 0, 0, 8),                        # the count
               (dst, 16, 2, 0, 8), (dst, 16, 0xFFFFFFFF, 0, 8),                # the visibility term
               (dst, 16, 0, 5, 5), (dst, 16, 0, 6, 5), (dst, 16, 0, 0, 9), (dst, 16, 0, 8, 9)]   # rows: empty, reversed, past the map
        for k, args in enumerate(bad):
            L.GPUX_OpBrdfLutGGX(g, *args)
            assert len(messages) == k + 1, (k, args[1:], messages)
        L.GPU_OpPrepareRenderPass(g, L.PBR_SunDepthRenderPass(sun))
        L.GPU_OpBeginRenderPass(g)
        L.GPUX_OpBrdfLutGGX(g, dst, 16, 0, 0, 8)                               # inside a render pass
        L.GPU_OpEndRenderPass(g)
        assert len(messages) == len(bad) + 1 and "inside a render pass" in messages[-1], messages
        L.GPU_GraphSubmit(g)
        L.GPU_GraphWait(g)
        assert L.GPUX_GraphTimedOpCount(g) == 0                                # nothing was recorded
        assert (pbrhip.read_mip(dst, 0) == SENTINEL).all()
        assert all(m.startswith("GPUX_OpBrdfLutGGX: ") for m in messages), messages
        L.GPUX_OpBrdfLutGGX(g, dst, 16, 0, 0, 8)                               # and a good one is one timed entry of that name
        L.GPU_GraphSubmit(g)
        L.GPU_GraphWait(g)
        assert [L.GPUX_GraphTimedOpName(g, i).decode() for i in range(L.GPUX_GraphTimedOpCount(g))] == ["K22.brdf_lut_ggx"]
        assert len(messages) == len(bad) + 1
    finally:
        L.GPUX_EnableOpTiming(0)
        L.GPUX_SetErrorHandler(None, None)
        L.GPU_DestroyGraph(g)
        L.PBR_DestroySunDepthPass(sun)
        for t in (dst, half4, cube, vol, wide):
            L.GPU_DestroyTexture(t)


# ---- the host layer and the pair through the lighting pass ----
def test_host_layer_is_one_op_over_all_rows(gpu):
    import pbrhip
    L = gpu
    tex = target(pbrhip.Format_RG16F, 37, 21)
    try:
        L.PBR_GenBRDFIntegrationMapGGX(tex, 64, B.CORRELATED)
        assert pbrhip.read_mip(tex, 0).tobytes() == bake(37, 21, 64, B.CORRELATED, fmt=pbrhip.Format_RG16F).tobytes()
    finally:
        L.GPU_DestroyTexture(tex)


def test_the_ggx_pair_through_the_lighting_pass(gpu):
    """K21's cube and K22's LUT shaded by the unchanged lighting pass equal the oracle fed the read-back maps (smoke()'s 1e-4
    criterion); after K1 overwrites the same LUT texture the next frame equals the oracle with THAT LUT: the 16-byte LUT twin the first
    frame built was dropped on the write"""
    import pbrhip
    import pbr_oracle as O
    from pbrhip import synth
    L = gpu
    env = synth.synth_env(64, seed=0x5EED0022)
    env_tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 64, 64, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), 16, 64, 32)
    W, H = 64, 36
    gbd = synth.synth_gbuffer_spheres(W, H)
    gb = pbrhip.PBR_GBuffer()
    L.PBR_MakeGBuffer(C.byref(gb), W, H, pbrhip.Format_RGBA32F)
    lp = g = None
    try:
        L.PBR_GenIrradianceMap(env_tex, maps.irradiance_map)
        L.PBR_GenPrefilteredEnvMapGGX(env_tex, maps.tex_specular_env_map, 1, 64)
        L.PBR_GenBRDFIntegrationMapGGX(maps.brdf_lut, 64, B.SCHLICK)
        for name, arr in (("base_color", gbd["base"]), ("normal", gbd["normal"]), ("orm", gbd["orm"]),
                          ("emissive", gbd["emissive"]), ("depth", gbd["depth"])):
            pbrhip.upload_mip(getattr(gb, name), 0, arr)
        lp = L.PBR_MakeLightingPass(C.byref(gb), C.byref(maps), W, H)
        glob = pbrhip.fill_globals(gbd["cam_pos"], aspect=W / H)
        og = O.OrcGlobals.from_buffer_copy(bytes(glob))
        n = maps.tex_specular_env_map.contents.mip_level_count
        ppyr = np.concatenate([pbrhip.read_mip(maps.tex_specular_env_map, m).ravel() for m in range(n)])
        irr = pbrhip.read_mip(maps.irradiance_map, 0)
        g = L.GPU_MakeGraph()

        def frame_and_oracle():
            L.PBR_RecordLightingPass(lp, g, C.byref(glob), 0, 0)
            L.GPU_GraphSubmit(g)
            L.GPU_GraphWait(g)
            lit = pbrhip.read_mip(gb.lighting_result, 0)
            lut = pbrhip.read_mip(maps.brdf_lut, 0).view(np.uint16)
            want = O.shade(og, gbd["base"], gbd["normal"], gbd["orm"], gbd["emissive"], gbd["depth"], flags=O.SHADE_IBL,
                           irradiance_cube=irr, prefiltered_pyr=ppyr, prefiltered_size=32, lut_half=lut)
            rel = float((np.abs(lit[..., :3].astype(np.float64) - want[..., :3]) / np.maximum(np.abs(want[..., :3]), 1e-2)).max())
            return lit, lut.copy(), rel

        lit_ggx, lut_ggx, rel_ggx = frame_and_oracle()
        want_lut = bake(64, 64, 64, B.SCHLICK, fmt=pbrhip.Format_RG16F)
        assert lut_ggx.tobytes() == want_lut.tobytes()                         # the bound LUT is K22's
        assert rel_ggx < 1e-4, rel_ggx
        L.PBR_GenBRDFIntegrationMap(maps.brdf_lut)                             # K1 into the same texture
        lit_k1, lut_k1, rel_k1 = frame_and_oracle()
        assert lut_k1.tobytes() != lut_ggx.tobytes()
        assert rel_k1 < 1e-4, rel_k1
        assert lit_k1.tobytes() != lit_ggx.tobytes()
        pbrhip.brdf_lut_ggx(maps.brdf_lut, 64, B.SCHLICK)                      # and K22 over K1's: the twin of K1's bytes goes too
        lit_again, lut_again, rel_again = frame_and_oracle()
        assert lut_again.tobytes() == lut_ggx.tobytes() and rel_again < 1e-4, rel_again
        assert lit_again.tobytes() == lit_ggx.tobytes()
    finally:
        if g:
            L.GPU_DestroyGraph(g)
        if lp:
            L.PBR_DestroyLightingPass(lp)
        L.PBR_DestroyGBuffer(C.byref(gb))
        L.PBR_DestroyIBLMaps(C.byref(maps))
        L.GPU_DestroyTexture(env_tex)


def test_demo_bakes_the_pair_with_the_keyword(gpu, tmp_path):
    """pbr_demo ... ggxpair 64 against ... ggx 64: the same line names, the same maps but the LUT, another frame"""
    import pbrhip
    from pbrhip import synth
    hdr = tmp_path / "cube_strip.hdr"
    hdr.write_bytes(synth.env_to_hdr_strip(synth.synth_env(64, seed=0x5EED0022), rle=True))
    exe = os.path.join(pbrhip.PKG_ROOT, "pbr_demo")
    base = [exe, str(hdr), "16", "64", "32", "8", "64", "36"]
    runs = []
    for extra in (["ggx", "64"], ["ggxpair", "64"]):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l.split() for l in out.stdout.splitlines()]
        assert lines[-1] == ["ok", "1"]
        runs.append(lines)
    ggx, pair = runs
    assert [l[:2] if l[0] == "time_ms" else l[:1] for l in ggx] == [l[:2] if l[0] == "time_ms" else l[:1] for l in pair]
    value = lambda lines, key: [l[1] for l in lines if l[0] == key]  # noqa: E731
    for key in ("env_mip0_sum", "irradiance_sum", "specular_mip0_sum", "specular_mip1_sum", "specular_mip2_sum"):
        assert value(ggx, key) == value(pair, key) and len(value(pair, key)) == 1, key
    assert value(ggx, "lut_bits_sum") != value(pair, "lut_bits_sum") and len(value(pair, "lut_bits_sum")) == 1
    assert subprocess.run(base + ["ggxpair", "0"], capture_output=True, text=True, timeout=120).returncode == 2
