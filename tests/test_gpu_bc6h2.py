"""K18 at its two-region quality on the GPU: the kernel against the numpy restatement of csrc/bc6h2_core.h (tests/bc6h2_ref.py), byte
for byte -- through GPUX_OpEncodeBC6HEx, the kernel's C entry point, hipGraph replay, a decode in the same graph, and the .dds writer /
loader of the host layer.  Levels are at most 260 x 260."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bc6h2_ref as R2  # noqa: E402
import bc6h_decode_ref as D  # noqa: E402
import bc6h_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

_CASES, _WANT = {}, {}


def case(name):
    if not _CASES:
        for n, lvl in R2.cases():
            lvl.setflags(write=False)
            _CASES[n] = lvl
        big = R.hdr_level(260, 260, 1, 260260)
        big.setflags(write=False)
        _CASES["flat260x260_f32"] = big
    return _CASES[name]


def want_of(name):
    """the contract's blocks of a case: computed once, shared, read-only"""
    if name not in _WANT:
        _WANT[name] = R2.encode2(case(name))
        _WANT[name].setflags(write=False)
    return _WANT[name]


def texture_of(level, mips=False):
    import pbrhip
    layers, h, w, _ = level.shape
    fmt = pbrhip.Format_RGBA32F if level.dtype == np.float32 else pbrhip.Format_RGBA16F
    flags = (pbrhip.TextureFlag_Cubemap if layers == 6 else 0) | (pbrhip.TextureFlag_HasMipmaps if mips else 0)
    return pbrhip.make_texture(fmt, w, h, flags, level)


def assert_blocks(label, got, want):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=1)).ravel()
    assert len(bad) == 0, (label, len(bad), bad[:5].tolist(), got[bad[:1]].tolist(), want[bad[:1]].tolist())


@pytest.mark.parametrize("name", ["cube1_f32", "cube2_f32", "cube3_f32", "cube5_f32", "cube12_f16", "cube68_f32", "flat20x12_f32", "flat20x12_f16",
                                  "flat260x260_f32", "partitions_f16", "crafted_f16", "crafted_f32", "edge_scene"])
def test_levels_equal_the_contract(gpu, name):
    """1, 2, 3, 5: clamped partial blocks, so subsets hold repeated texels; 12 / 68: both source formats, 17 blocks per row so rows do
    not align to a wave; 260 x 260: 4225 blocks, several workgroups, the last ragged; the partition strip: every partition; the crafted
    strip: every path of the contract (tests/bc6h2_ref.py crafted_blocks, bc6h_ref.hostile_blocks); the scene: hard edges"""
    import pbrhip
    lvl = case(name)
    tex = texture_of(lvl)
    try:
        assert gpu.GPUX_BC6HMipBytes(tex, 0) == R.level_bytes(lvl.shape[2], lvl.shape[1], lvl.shape[0])
        got = pbrhip.encode_bc6h(tex, 0, pbrhip.GPUX_BC6H_TwoRegions)
        assert_blocks(name, got, want_of(name))
        assert D.decode(got).max() <= R.MAX_CODE                              # never Inf
    finally:
        gpu.GPU_DestroyTexture(tex)


def test_quality_zero_records_the_one_region_op(gpu):
    """GPUX_OpEncodeBC6HEx at GPUX_BC6H_OneRegion: GPUX_OpEncodeBC6H's bytes, which are bc6h_ref.encode's; and the two qualities differ"""
    import pbrhip
    L = gpu
    lvl = case("cube12_f16")
    tex = texture_of(lvl)
    nbytes = R.level_bytes(12, 12, 6)
    try:
        plain = pbrhip.encode_bc6h(tex, 0)
        ex0 = pbrhip._read_back(lambda g, buf: L.GPUX_OpEncodeBC6HEx(g, tex, 0, buf, 0, pbrhip.GPUX_BC6H_OneRegion), nbytes)
        assert ex0 == plain.tobytes() == R.encode(lvl).tobytes()
        assert pbrhip.encode_bc6h(tex, 0, 1).tobytes() != ex0
    finally:
        L.GPU_DestroyTexture(tex)


def test_op_mip_offset_and_untouched_bytes(gpu):
    """a mip other than 0 of a cube with a chain (20, 10, 5, 2, 1), at a non-zero offset; the bytes around the range stay as they were"""
    import pbrhip
    L = gpu
    tex = texture_of(case("cube20_f32"), mips=True)
    assert tex.contents.mip_level_count == 5
    pad = 48
    try:
        for mip in (2, 1, 4):
            n = max(1, 20 >> mip)
            nbytes = R.level_bytes(n, n, 6)
            want = R2.encode2(pbrhip.read_mip(tex, mip))
            buf = L.GPU_MakeBuffer(pad + nbytes + 32, pbrhip.BufferFlag_CPU, None)
            g = L.GPU_MakeGraph()
            C.memset(buf.contents.data, 0xA5, pad + nbytes + 32)
            L.GPUX_OpEncodeBC6HEx(g, tex, mip, buf, pad, 1)
            L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
            raw = C.string_at(buf.contents.data, pad + nbytes + 32)
            L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(buf)
            assert raw[:pad] == b"\xa5" * pad and raw[pad + nbytes:] == b"\xa5" * 32, mip
            assert_blocks(f"mip {mip}", np.frombuffer(raw[pad:pad + nbytes], np.uint8).reshape(-1, 16), want)
    finally:
        L.GPU_DestroyTexture(tex)


def test_op_twice_in_a_graph_submitted_twice(gpu):
    """two records of the op in one graph, the graph recorded and submitted twice, plain and under GPUX_SetGraphReplay(1): the same bytes"""
    import pbrhip
    L = gpu
    tex = texture_of(case("cube68_f32"))
    nbytes = R.level_bytes(68, 68, 6)
    buf = L.GPU_MakeBuffer(2 * nbytes, pbrhip.BufferFlag_CPU, None)
    results = []
    try:
        for replay in (0, 1):
            L.GPUX_SetGraphReplay(replay)
            g = L.GPU_MakeGraph()
            for _ in range(2):
                C.memset(buf.contents.data, 0, 2 * nbytes)
                L.GPUX_OpEncodeBC6HEx(g, tex, 0, buf, 0, 1)
                L.GPUX_OpEncodeBC6HEx(g, tex, 0, buf, nbytes, 1)
                L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
                raw = C.string_at(buf.contents.data, 2 * nbytes)
                results += [raw[:nbytes], raw[nbytes:]]
            s = [C.c_uint64() for _ in range(3)]
            L.GPUX_GraphReplayStats(g, *[C.byref(v) for v in s])
            print(f"replay {replay}: launches {s[0].value}, updates {s[1].value}, instantiations {s[2].value}")
            assert s[0].value == (2 if replay else 0)
            L.GPU_DestroyGraph(g)
    finally:
        L.GPUX_SetGraphReplay(-1)
        L.GPU_DestroyBuffer(buf); L.GPU_DestroyTexture(tex)
    assert len(results) == 8 and all(r == results[0] for r in results)
    assert_blocks("twice, twice", np.frombuffer(results[7], np.uint8).reshape(-1, 16), want_of("cube68_f32"))


def test_encode_and_decode_in_one_graph(gpu):
    """quality 1 into a device buffer and GPUX_OpDecodeBC6H from it into an RGBA32F cube, one graph: the texels are what the independent
    decoder makes of the restatement's blocks, bit for bit"""
    import pbrhip
    L = gpu
    tex = texture_of(case("cube12_f16"))
    back = pbrhip.make_texture(pbrhip.Format_RGBA32F, 12, 12, pbrhip.TextureFlag_Cubemap)
    nbytes = R.level_bytes(12, 12, 6)
    dev = L.GPU_MakeBuffer(nbytes, pbrhip.BufferFlag_GPU, None)
    g = L.GPU_MakeGraph()
    try:
        L.GPUX_OpEncodeBC6HEx(g, tex, 0, dev, 0, 1)
        L.GPUX_OpDecodeBC6H(g, dev, 0, back, 0)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        got = pbrhip.read_mip(back, 0)
        want = D.level_rgba(want_of("cube12_f16"), 12, 12, 6, True)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    finally:
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(dev); L.GPU_DestroyTexture(back); L.GPU_DestroyTexture(tex)


def test_op_refuses_bad_arguments(gpu):
    """with an error handler installed a refused record reports once, naming GPUX_OpEncodeBC6HEx, and records nothing"""
    import pbrhip
    L = gpu
    messages = []
    handler = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)(lambda msg, user: messages.append(msg.decode()))
    tex = texture_of(case("cube3_f32"))                                       # one block a face: 96 bytes
    lut = pbrhip.make_texture(pbrhip.Format_RG16F, 4, 4, 0, np.zeros((4, 4, 2), np.float16))
    buf = L.GPU_MakeBuffer(256, pbrhip.BufferFlag_CPU, None)
    g = L.GPU_MakeGraph()
    L.GPUX_SetErrorHandler(C.cast(handler, C.c_void_p), None)
    try:
        C.memset(buf.contents.data, 0x5A, 256)
        L.GPUX_OpEncodeBC6HEx(g, tex, 0, buf, 0, 2)         # no such quality
        L.GPUX_OpEncodeBC6HEx(g, tex, 0, buf, 0, 0xFFFFFFFF)
        L.GPUX_OpEncodeBC6HEx(g, tex, 0, buf, 8, 1)         # offset not a multiple of 16
        L.GPUX_OpEncodeBC6HEx(g, tex, 0, buf, 176, 1)       # 96 bytes do not fit behind 176
        L.GPUX_OpEncodeBC6HEx(g, lut, 0, buf, 0, 1)         # RG16F
        L.GPUX_OpEncodeBC6HEx(g, tex, 1, buf, 0, 1)         # no such mip
        L.GPUX_OpEncodeBC6HEx(g, None, 0, buf, 0, 1)
        L.GPUX_OpEncodeBC6HEx(g, tex, 0, None, 0, 1)
        assert len(messages) == 8 and all("GPUX_OpEncodeBC6HEx" in m for m in messages), messages
        assert "quality" in messages[0] and "quality" in messages[1] and "multiple of 16" in messages[2] and "too small" in messages[3] and "RGBA32F / RGBA16F" in messages[4]
        L.GPUX_OpEncodeBC6HEx(g, tex, 0, buf, 160, 1)       # the last place where the 96 bytes fit
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        raw = C.string_at(buf.contents.data, 256)
        assert raw[:160] == b"\x5a" * 160 and raw[160:] == want_of("cube3_f32").tobytes()     # only the accepted record ran
        assert len(messages) == 8
    finally:
        L.GPUX_SetErrorHandler(None, None)
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(buf); L.GPU_DestroyTexture(tex); L.GPU_DestroyTexture(lut)


def test_kernel_entry_point_checks_its_arguments(gpu):
    """pbrk_bc6h_encode2 returns pbrk_bc6h_encode's codes for the same bad arguments and launches nothing; the valid call afterwards
    writes the contract's bytes"""
    import pbrhip
    L = gpu
    OK, E_ARG, E_FORMAT = 0, -1, -2
    F32, F16, RG16F = 4, 3, 1                                                  # PBRK_FMT_*
    tex = texture_of(case("cube5_f32"))
    nbytes = R.level_bytes(5, 5, 6)
    buf = L.GPU_MakeBuffer(nbytes + 16, pbrhip.BufferFlag_CPU, None)
    try:
        src, dst = L.GPUX_TextureDevicePtr(tex, 0), L.GPUX_BufferDevicePtr(buf)
        C.memset(buf.contents.data, 0x3C, nbytes + 16)
        bad = [((None, F32, 5, 5, 6, dst), E_ARG), ((src, F32, 5, 5, 6, None), E_ARG), ((src, F32, 0, 5, 6, dst), E_ARG), ((src, F32, 5, 0, 6, dst), E_ARG),
               ((src, F32, 16385, 5, 6, dst), E_ARG), ((src, F32, 5, 16385, 6, dst), E_ARG), ((src, F32, 5, 5, 0, dst), E_ARG), ((src, F32, -5, 5, 6, dst), E_ARG),
               ((src, F32, 5, 5, 65536, dst), E_ARG), ((src, RG16F, 5, 5, 6, dst), E_FORMAT), ((src, 0, 5, 5, 6, dst), E_FORMAT), ((src, 99, 5, 5, 6, dst), E_FORMAT),
               ((src + 8, F32, 5, 5, 6, dst), E_ARG), ((src + 4, F16, 5, 5, 6, dst), E_ARG), ((src, F32, 5, 5, 6, dst + 8), E_ARG)]
        for args, want in bad:
            assert L.pbrk_bc6h_encode2(*args, None) == want == L.pbrk_bc6h_encode(*args, None), args
        L.GPU_WaitUntilIdle()
        assert C.string_at(buf.contents.data, nbytes + 16) == b"\x3c" * (nbytes + 16)          # nothing was launched
        assert L.pbrk_bc6h_encode2(src, F32, 5, 5, 6, dst + 16, None) == OK
        L.GPU_WaitUntilIdle()
        raw = C.string_at(buf.contents.data, nbytes + 16)
        assert raw[:16] == b"\x3c" * 16
        assert_blocks("entry point", np.frombuffer(raw[16:], np.uint8).reshape(-1, 16), want_of("cube5_f32"))
    finally:
        L.GPU_DestroyBuffer(buf); L.GPU_DestroyTexture(tex)


def test_two_region_dds_of_a_cube_with_its_chain(gpu):
    """PBR_DDS_OUT_BC6H_UF16_2R: the container of the one-region file (DXGI 95, the same offsets), every level's blocks the contract's,
    and the BC6H loader takes it as it is"""
    import pbrhip
    L = gpu
    tex = texture_of(case("cube20_f32"), mips=True)
    back = None
    try:
        data = pbrhip.encode_dds(tex, 0, 0, pbrhip.PBR_DDS_OUT_BC6H_UF16_2R)
        one = pbrhip.encode_dds(tex, 0, 0, pbrhip.PBR_DDS_OUT_BC6H_UF16)
        info, info1 = pbrhip.parse_dds_ex(data), pbrhip.parse_dds_ex(one)
        assert (info.dxgi_format, info.width, info.height, info.layers, info.level_count) == (95, 20, 20, 6, 5)
        assert len(data) == len(one) and data[:148] == one[:148] and data != one
        for m in range(5):
            assert info.level_size[m] == info1.level_size[m]
            level = pbrhip.read_mip(tex, m)
            want = R2.encode2(level).reshape(6, -1)
            assert want.shape[1] == info.level_size[m]
            for l in range(6):
                o = info.level_offset[l][m]
                assert o == info1.level_offset[l][m]
                assert data[o:o + info.level_size[m]] == want[l].tobytes(), (m, l)
        back = L.PBR_MakeTextureFromBC6HDDSMemory(data, len(data), pbrhip.Format_RGBA32F)
        assert back
        b = back.contents
        assert (b.format, b.width, b.height, b.layer_count, b.mip_level_count) == (pbrhip.Format_RGBA32F, 20, 20, 6, 5)
        for m in range(5):
            n = max(1, 20 >> m)
            want = D.level_rgba(R2.encode2(pbrhip.read_mip(tex, m)), n, n, 6, True)
            assert np.array_equal(pbrhip.read_mip(back, m).view(np.uint32), want.view(np.uint32)), m
    finally:
        L.GPU_DestroyTexture(tex); L.GPU_DestroyTexture(back)


def test_demo_saves_its_bake_at_two_regions(gpu, tmp_path):
    """pbr_demo ... dds2 PREFIX: the specular file is PBR_EncodeTextureDDS(..., PBR_DDS_OUT_BC6H_UF16_2R) of the same bake driven from
    here, the other two files are what `dds` writes, and every other line of the demo's output is what it prints without it"""
    import subprocess
    import pbrhip
    from pbrhip import synth
    L = gpu
    hdr = tmp_path / "cube_strip.hdr"
    hdr.write_bytes(synth.env_to_hdr_strip(synth.synth_env(64, seed=0x5EED0018), rle=True))
    exe = os.path.join(pbrhip.PKG_ROOT, "pbr_demo")
    sizes = ["32", "256", "64", "16", "320", "180"]
    prefix1, prefix2 = str(tmp_path / "one"), str(tmp_path / "two")

    def lines(extra):
        out = subprocess.run([exe, str(hdr), *sizes, *extra], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return [l for l in out.stdout.splitlines() if not l.startswith("time_ms")]

    with_dds, with_dds2 = lines(["dds", prefix1]), lines(["dds2", prefix2])
    assert with_dds2 == with_dds and with_dds2[-1] == "ok 1"                  # the sizes printed as dds_bytes are the same too
    env = L.PBR_MakeTextureFromHDRIFile(str(hdr).encode())
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), 32, 256, 64)
    try:
        L.PBR_GenPrefilteredEnvMap(env, maps.tex_specular_env_map, 16)
        want = pbrhip.encode_dds(maps.tex_specular_env_map, 0, 3, pbrhip.PBR_DDS_OUT_BC6H_UF16_2R)      # 64, 32, 16
    finally:
        L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(env)
    got = open(prefix2 + "_specular.dds", "rb").read()
    assert got == want and got != open(prefix1 + "_specular.dds", "rb").read()
    for name in ("irradiance", "lut"):
        assert open(f"{prefix2}_{name}.dds", "rb").read() == open(f"{prefix1}_{name}.dds", "rb").read(), name
    info = pbrhip.parse_dds_ex(got)
    assert (info.dxgi_format, info.width, info.layers, info.level_count) == (95, 64, 6, 3)
