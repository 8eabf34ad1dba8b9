"""K18 on the GPU: the BC6H encode kernel against the numpy restatement of the contract (tests/bc6h_ref.py), byte for byte -- through
the graph op, the kernel's C entry point, hipGraph replay and the .dds writer / loader of the host layer.  Levels are at most 260 x 260."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bc6h_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

_CASES, _WANT = {}, {}


def case(name):
    if not _CASES:
        for n, lvl in R.cases():
            lvl.setflags(write=False)
            _CASES[n] = lvl
    return _CASES[name]


def want_of(name):
    """the contract's blocks of a case: computed once, shared, read-only"""
    if name not in _WANT:
        _WANT[name] = R.encode(case(name))
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


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("n", R.CUBE_FACES)
def test_cube_levels_equal_the_contract(gpu, n, fmt):
    """1 .. 4: one block, the first three with clamped edges; 5, 6: clamped edges in the second block; 12, 20: whole blocks; 68: 17
    blocks per row, so the rows of a layer do not align to a wave; 260: 4225 blocks per layer, 17 workgroups, the last one ragged"""
    import pbrhip
    name = f"cube{n}_{fmt}"
    tex = texture_of(case(name))
    try:
        assert gpu.GPUX_BC6HMipBytes(tex, 0) == R.level_bytes(n, n, 6)
        assert_blocks(name, pbrhip.encode_bc6h(tex, 0), want_of(name))
    finally:
        gpu.GPU_DestroyTexture(tex)


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("w,h", R.FLAT_LEVELS)
def test_flat_levels_equal_the_contract(gpu, w, h, fmt):
    import pbrhip
    name = f"flat{w}x{h}_{fmt}"
    tex = texture_of(case(name))
    try:
        assert gpu.GPUX_BC6HMipBytes(tex, 0) == R.level_bytes(w, h, 1)
        assert_blocks(name, pbrhip.encode_bc6h(tex, 0), want_of(name))
    finally:
        gpu.GPU_DestroyTexture(tex)


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_hostile_texels_equal_the_contract(gpu, fmt):
    """negative values, -0, NaN, +-Inf, 1e30, fp32 and fp16 subnormals, 65504, 65520, an all-equal and an all-zero block, texel 0 the
    brightest (the swap path), red rising as blue falls (candidate 2), a noisy block (the inset); tests/bc6h_ref.py hostile_blocks"""
    import pbrhip
    name = f"hostile_{fmt}"
    tex = texture_of(case(name))
    try:
        got = pbrhip.encode_bc6h(tex, 0)
        assert_blocks(name, got, want_of(name))
        assert np.isfinite(R.decode_level(got, case(name).shape[2], 4, 1)).all()
    finally:
        gpu.GPU_DestroyTexture(tex)


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
            assert L.GPUX_BC6HMipBytes(tex, mip) == nbytes
            want = R.encode(pbrhip.read_mip(tex, mip))
            buf = L.GPU_MakeBuffer(pad + nbytes + 32, pbrhip.BufferFlag_CPU, None)
            g = L.GPU_MakeGraph()
            C.memset(buf.contents.data, 0xA5, pad + nbytes + 32)
            L.GPUX_OpEncodeBC6H(g, tex, mip, buf, pad)
            L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
            raw = C.string_at(buf.contents.data, pad + nbytes + 32)
            L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(buf)
            assert raw[:pad] == b"\xa5" * pad and raw[pad + nbytes:] == b"\xa5" * 32, mip
            assert_blocks(f"mip {mip}", np.frombuffer(raw[pad:pad + nbytes], np.uint8).reshape(-1, 16), want)
        assert L.GPUX_BC6HMipBytes(tex, 5) == 0
    finally:
        L.GPU_DestroyTexture(tex)


def test_op_in_a_device_buffer_ordered_with_a_copy(gpu):
    """the op writes a GPU buffer and a buffer copy recorded after it in the same graph reads the blocks: a plain graph op"""
    import pbrhip
    L = gpu
    tex = texture_of(case("cube12_f16"))
    nbytes = R.level_bytes(12, 12, 6)
    dev = L.GPU_MakeBuffer(nbytes, pbrhip.BufferFlag_GPU, None)
    host = L.GPU_MakeBuffer(nbytes, pbrhip.BufferFlag_CPU, None)
    g = L.GPU_MakeGraph()
    try:
        L.GPUX_OpEncodeBC6H(g, tex, 0, dev, 0)
        L.GPU_OpCopyBufferToBuffer(g, dev, host, 0, 0, nbytes)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        got = np.frombuffer(C.string_at(host.contents.data, nbytes), np.uint8).reshape(-1, 16)
        assert_blocks("device buffer", got, want_of("cube12_f16"))
    finally:
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(dev); L.GPU_DestroyBuffer(host); L.GPU_DestroyTexture(tex)


def test_graph_replay_gives_the_same_bytes(gpu):
    """the op is captured under GPUX_SetGraphReplay(1); instantiation and the updated replay give the plain bytes"""
    import pbrhip
    L = gpu
    tex = texture_of(case("cube68_f32"))
    nbytes = R.level_bytes(68, 68, 6)
    buf = L.GPU_MakeBuffer(nbytes, pbrhip.BufferFlag_CPU, None)
    results = []
    try:
        for replay in (0, 1):
            L.GPUX_SetGraphReplay(replay)
            g = L.GPU_MakeGraph()
            for _ in range(2):
                C.memset(buf.contents.data, 0, nbytes)
                L.GPUX_OpEncodeBC6H(g, tex, 0, buf, 0)
                L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
                results.append(C.string_at(buf.contents.data, nbytes))
            s = [C.c_uint64() for _ in range(3)]
            L.GPUX_GraphReplayStats(g, *[C.byref(v) for v in s])
            print(f"replay {replay}: launches {s[0].value}, updates {s[1].value}, instantiations {s[2].value}")
            assert s[0].value == (2 if replay else 0)
            L.GPU_DestroyGraph(g)
    finally:
        L.GPUX_SetGraphReplay(-1)
        L.GPU_DestroyBuffer(buf); L.GPU_DestroyTexture(tex)
    assert all(r == results[0] for r in results)
    assert_blocks("under replay", np.frombuffer(results[3], np.uint8).reshape(-1, 16), want_of("cube68_f32"))


def test_op_refuses_bad_arguments(gpu):
    """with an error handler installed a refused record reports and records nothing: only the accepted op of the graph runs"""
    import pbrhip
    L = gpu
    messages = []
    handler = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)(lambda msg, user: messages.append(msg.decode()))
    tex = texture_of(case("cube4_f32"))
    lut = pbrhip.make_texture(pbrhip.Format_RG16F, 4, 4, 0, np.zeros((4, 4, 2), np.float16))
    buf = L.GPU_MakeBuffer(256, pbrhip.BufferFlag_CPU, None)
    g = L.GPU_MakeGraph()
    L.GPUX_SetErrorHandler(C.cast(handler, C.c_void_p), None)
    try:
        C.memset(buf.contents.data, 0x5A, 256)
        L.GPUX_OpEncodeBC6H(g, tex, 1, buf, 0)          # no such mip
        L.GPUX_OpEncodeBC6H(g, tex, 0, buf, 8)          # offset not a multiple of 16
        L.GPUX_OpEncodeBC6H(g, tex, 0, buf, 176)        # 96 bytes do not fit behind 176
        L.GPUX_OpEncodeBC6H(g, lut, 0, buf, 0)          # RG16F
        L.GPUX_OpEncodeBC6H(g, None, 0, buf, 0)
        L.GPUX_OpEncodeBC6H(g, tex, 0, None, 0)
        assert len(messages) == 6 and all("GPUX_OpEncodeBC6H" in m for m in messages), messages
        L.GPUX_OpEncodeBC6H(g, tex, 0, buf, 160)        # the last place where the 96 bytes fit
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        raw = C.string_at(buf.contents.data, 256)
        assert raw[:160] == b"\x5a" * 160 and raw[160:] == want_of("cube4_f32").tobytes()     # only the accepted record ran
        assert len(messages) == 6
        assert L.GPUX_BC6HMipBytes(lut, 0) == 0 and L.GPUX_BC6HMipBytes(None, 0) == 0
    finally:
        L.GPUX_SetErrorHandler(None, None)
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(buf); L.GPU_DestroyTexture(tex); L.GPU_DestroyTexture(lut)


def test_kernel_entry_point_checks_its_arguments(gpu):
    """pbrk_bc6h_encode returns an error and launches nothing for a null pointer, an extent of 0 or above 16384, another format,
    a misaligned pointer; the valid call afterwards writes the contract's bytes"""
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
               ((src, RG16F, 5, 5, 6, dst), E_FORMAT), ((src, 0, 5, 5, 6, dst), E_FORMAT), ((src, 99, 5, 5, 6, dst), E_FORMAT),
               ((src + 8, F32, 5, 5, 6, dst), E_ARG), ((src + 4, F16, 5, 5, 6, dst), E_ARG), ((src, F32, 5, 5, 6, dst + 8), E_ARG)]
        for args, want in bad:
            assert L.pbrk_bc6h_encode(*args, None) == want, args
        L.GPU_WaitUntilIdle()
        assert C.string_at(buf.contents.data, nbytes + 16) == b"\x3c" * (nbytes + 16)          # nothing was launched
        assert L.pbrk_bc6h_level_bytes(5, 5, 6) == nbytes and L.pbrk_bc6h_level_bytes(0, 5, 6) == 0 and L.pbrk_bc6h_level_bytes(16384, 16384, 6) == 6 * 4096 * 4096 * 16
        assert L.pbrk_bc6h_encode(src, F32, 5, 5, 6, dst + 16, None) == OK
        L.GPU_WaitUntilIdle()
        raw = C.string_at(buf.contents.data, nbytes + 16)
        assert raw[:16] == b"\x3c" * 16
        assert_blocks("entry point", np.frombuffer(raw[16:], np.uint8).reshape(-1, 16), want_of("cube5_f32"))
    finally:
        L.GPU_DestroyBuffer(buf); L.GPU_DestroyTexture(tex)


@pytest.fixture(scope="module")
def bake(gpu):
    """a small job: env 64^2 -> specular 16^2 with mips, irradiance 8^2, LUT 16^2"""
    import pbrhip
    from pbrhip import synth
    L = gpu
    env = synth.synth_env(64, seed=0x5EED0B06)
    env_tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 64, 64, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), 8, 16, 16)
    L.PBR_GenPrefilteredEnvMap(env_tex, maps.tex_specular_env_map, 1)
    L.PBR_GenIrradianceMap(env_tex, maps.irradiance_map)
    L.PBR_GenBRDFIntegrationMap(maps.brdf_lut)
    yield maps
    L.PBR_DestroyIBLMaps(C.byref(maps))
    L.GPU_DestroyTexture(env_tex)


def test_float_dds_round_trip_of_a_bake(gpu, bake, tmp_path):
    """every map written as a float .dds and loaded back: format, extents, layers, levels and every level's bytes are the texture's"""
    import pbrhip
    L = gpu
    for name, tex, dxgi in (("specular", bake.tex_specular_env_map, 2), ("irradiance", bake.irradiance_map, 2), ("lut", bake.brdf_lut, 34)):
        path = str(tmp_path / f"bake_{name}.dds")
        pbrhip.write_dds(path, tex)
        t = tex.contents
        data = open(path, "rb").read()
        info = pbrhip.parse_dds_ex(data)
        assert (info.dxgi_format, info.width, info.height, info.layers, info.level_count) == (dxgi, t.width, t.height, t.layer_count, t.mip_level_count), name
        assert data == pbrhip.encode_dds(tex)
        for m in range(t.mip_level_count):                                     # face-major in the file, level-major in the texture
            level = pbrhip.read_mip_bytes(tex, m)
            per = len(level) // t.layer_count
            assert per == info.level_size[m]
            for l in range(t.layer_count):
                o = info.level_offset[l][m]
                assert data[o:o + per] == level[l * per:(l + 1) * per], (name, m, l)
        back = pbrhip.make_texture_from_float_dds_file(path)
        try:
            b = back.contents
            assert (b.format, b.width, b.height, b.layer_count, b.mip_level_count) == (t.format, t.width, t.height, t.layer_count, t.mip_level_count), name
            for m in range(t.mip_level_count):
                assert pbrhip.read_mip_bytes(back, m) == pbrhip.read_mip_bytes(tex, m), (name, m)
        finally:
            L.GPU_DestroyTexture(back)


def test_float_dds_round_trip_of_a_flat_chain_and_no_partial_chain(gpu):
    """a 2-D 24 x 12 RGBA16F texture with its chain (24 x 12, 12 x 6, 6 x 3, 3 x 1) written as it is and loaded back: every level's bytes;
    the same texture written with two of its four levels is refused: the float loader takes a whole chain or one level"""
    import pbrhip
    L = gpu
    tex = pbrhip.make_texture(pbrhip.Format_RGBA16F, 24, 12, pbrhip.TextureFlag_HasMipmaps)
    back = None
    try:
        assert tex.contents.mip_level_count == 4
        rng = np.random.default_rng(0x5EED2412)
        for m in range(4):
            pbrhip.upload_mip(tex, m, rng.integers(0, 0x7C00, (max(1, 12 >> m), 24 >> m, 4), dtype=np.uint16))
        data = pbrhip.encode_dds(tex)
        info = pbrhip.parse_dds_ex(data)
        assert (info.dxgi_format, info.width, info.height, info.layers, info.level_count) == (10, 24, 12, 1, 4)
        back = L.PBR_MakeTextureFromFloatDDSMemory(data, len(data))
        assert back
        b = back.contents
        assert (b.format, b.width, b.height, b.layer_count, b.mip_level_count) == (pbrhip.Format_RGBA16F, 24, 12, 1, 4)
        for m in range(4):
            level = pbrhip.read_mip_bytes(tex, m)
            assert len(level) == info.level_size[m] and data[info.level_offset[0][m]:][:len(level)] == level, m
            assert pbrhip.read_mip_bytes(back, m) == level, m
        part = pbrhip.encode_dds(tex, 0, 2)
        assert pbrhip.parse_dds_ex(part).level_count == 2
        assert not L.PBR_MakeTextureFromFloatDDSMemory(part, len(part))
    finally:
        L.GPU_DestroyTexture(tex); L.GPU_DestroyTexture(back)


def test_rgba16f_dds_is_the_contract_conversion(gpu, bake):
    """RGBA32F narrowed on the host: round to nearest even, sign and Inf kept; a sub-range of the chain"""
    import pbrhip
    tex = bake.tex_specular_env_map
    data = pbrhip.encode_dds(tex, 1, 3, pbrhip.PBR_DDS_OUT_RGBA16F)
    info = pbrhip.parse_dds_ex(data)
    assert (info.dxgi_format, info.width, info.layers, info.level_count) == (10, 8, 6, 3)
    for m in range(3):
        level = pbrhip.read_mip(tex, 1 + m)
        want = R.f16_from_f32(level.view(np.uint32)).astype(np.uint16)
        for l in range(6):
            o = info.level_offset[l][m]
            got = np.frombuffer(data[o:o + info.level_size[m]], np.uint16).reshape(want.shape[1:])
            assert np.array_equal(got, want[l]), (m, l)


def test_bc6h_dds_of_the_specular_cube(gpu, bake, tmp_path):
    """the file's payload is the contract's encode of each level, face-major; it cannot be loaded back (out of scope)"""
    import pbrhip
    tex = bake.tex_specular_env_map
    path = str(tmp_path / "bake_specular_bc6h.dds")
    pbrhip.write_dds(path, tex, 0, 0, pbrhip.PBR_DDS_OUT_BC6H_UF16)
    data = open(path, "rb").read()
    info = pbrhip.parse_dds_ex(data)
    levels = tex.contents.mip_level_count
    assert (info.dxgi_format, info.width, info.height, info.layers, info.level_count) == (95, 16, 16, 6, levels)
    end = 148
    for l in range(6):
        for m in range(levels):
            assert info.level_offset[l][m] == end
            end += info.level_size[m]
    assert end == len(data)
    for m in range(levels):
        level = pbrhip.read_mip(tex, m)
        want = R.encode(level).reshape(6, -1)
        assert want.shape[1] == info.level_size[m]
        for l in range(6):
            o = info.level_offset[l][m]
            assert data[o:o + info.level_size[m]] == want[l].tobytes(), (m, l)
        assert_blocks(f"op, level {m}", pbrhip.encode_bc6h(tex, m), R.encode(level))
    with pytest.raises(RuntimeError):
        pbrhip.make_texture_from_float_dds_file(path)


def test_demo_saves_its_bake_as_dds(gpu, tmp_path):
    """pbr_demo ... dds PREFIX: the three files are what PBR_EncodeTextureDDS gives for the same bake driven from here (the specular cube
    as BC6H down to min_size, irradiance and LUT as they are); every other line of the demo's output is what it prints without it"""
    import subprocess
    import pbrhip
    from pbrhip import synth
    L = gpu
    hdr = tmp_path / "cube_strip.hdr"
    hdr.write_bytes(synth.env_to_hdr_strip(synth.synth_env(64, seed=0x5EED0018), rle=True))
    exe = os.path.join(pbrhip.PKG_ROOT, "pbr_demo")
    sizes = ["32", "256", "64", "16", "320", "180"]                     # the sizes of the demo's end-to-end test
    prefix = str(tmp_path / "bake")

    def lines(extra):
        out = subprocess.run([exe, str(hdr), *sizes, *extra], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return [l for l in out.stdout.splitlines() if not l.startswith("time_ms")]

    plain, with_dds = lines([]), lines(["dds", prefix])
    assert [l for l in with_dds if not l.startswith("dds_bytes")] == plain and plain[-1] == "ok 1"
    env = L.PBR_MakeTextureFromHDRIFile(str(hdr).encode())
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), 32, 256, 64)
    try:
        L.PBR_GenIrradianceMap(env, maps.irradiance_map)
        L.PBR_GenPrefilteredEnvMap(env, maps.tex_specular_env_map, 16)
        L.PBR_GenBRDFIntegrationMap(maps.brdf_lut)
        want = {"specular": pbrhip.encode_dds(maps.tex_specular_env_map, 0, 3, pbrhip.PBR_DDS_OUT_BC6H_UF16),      # 64, 32, 16
                "irradiance": pbrhip.encode_dds(maps.irradiance_map), "lut": pbrhip.encode_dds(maps.brdf_lut)}
    finally:
        L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(env)
    printed = {l.split()[1]: int(l.split()[2]) for l in with_dds if l.startswith("dds_bytes")}
    for name, data in want.items():
        got = open(f"{prefix}_{name}.dds", "rb").read()
        assert got == data and printed[name] == len(data), name
    info = pbrhip.parse_dds_ex(want["specular"])
    assert (info.dxgi_format, info.width, info.layers, info.level_count) == (95, 64, 6, 3)
    assert pbrhip.parse_dds_ex(want["lut"]).dxgi_format == 34
