"""K19 on the GPU: the BC6H decode kernel against the numpy restatement of the contract (tests/bc6h_decode_ref.py), every byte equal in
both target formats -- through the graph op, the kernel's C entry point, hipGraph replay, the .dds loader of the host layer, the
lighting pass and pbr_demo.  Levels are at most 260 x 260, but for the three around the threshold between the two kernels (17 MB each)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bc6h_decode_ref as D  # noqa: E402
import bc6h_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = ("f32", "f16")
_BLOCKS, _WANT = {}, {}


def blocks_of(name):
    """name -> (blocks, w, h, layers): computed once, shared, read-only.  mixed:<w>x<h>x<layers>: a random mode per block;
    mode:<M>: 20^2 cube of mode M throughout; enc:<w>x<h>x<layers>: the encode contract's blocks of HDR content"""
    if name not in _BLOCKS:
        kind, _, arg = name.partition(":")
        if kind == "mode":
            w, h, layers = 20, 20, 6
            b = D.random_blocks(layers * 25, 0xD00 + int(arg), mode=int(arg))
        else:
            w, h, layers = (int(v) for v in arg.split("x"))
            n = layers * ((w + 3) // 4) * ((h + 3) // 4)
            b = D.random_blocks(n, 1000 * w + h) if kind == "mixed" else R.encode(R.hdr_level(w, h, layers, 7 * w + h))
        b.setflags(write=False)
        _BLOCKS[name] = (b, w, h, layers)
    return _BLOCKS[name]


def want_of(name, fmt):
    """the contract's level as the kernel stores it: uint32 (RGBA32F bits) or uint16 (RGBA16F bits) [layers][h][w][4]"""
    if name not in _WANT:
        b, w, h, layers = blocks_of(name)
        half = D.level_rgba(b, w, h, layers, False)
        wide = D.level_rgba(b, w, h, layers, True).view(np.uint32)
        half.setflags(write=False); wide.setflags(write=False)
        _WANT[name] = {"f16": half, "f32": wide}
    return _WANT[name][fmt]


def gpu_format(fmt):
    import pbrhip
    return pbrhip.Format_RGBA32F if fmt == "f32" else pbrhip.Format_RGBA16F


def bits(level):
    level = np.ascontiguousarray(level)
    return level.view(np.uint32) if level.dtype == np.float32 else level.view(np.uint16)


def assert_level(label, got, want):
    got = bits(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (label, len(bad), bad[:4].tolist(), hex(int(got[tuple(bad[0])])), hex(int(want[tuple(bad[0])])))


def decode_case(name, fmt):
    import pbrhip
    b, w, h, layers = blocks_of(name)
    assert_level(f"{name} {fmt}", pbrhip.decode_bc6h(b, w, h, layers, gpu_format(fmt)), want_of(name, fmt))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", R.CUBE_FACES)
def test_cube_levels_of_mixed_modes_equal_the_contract(gpu, n, fmt):
    """1 .. 3, 5, 6: partial blocks, the narrow path; 4, 12, 20: whole blocks; 68: 17 blocks per row, a ragged wave; 260: 65 blocks
    per row, two workgroups per block row.  A random mode per block, so the modes mix inside every wave"""
    decode_case(f"mixed:{n}x{n}x6", fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", R.FLAT_LEVELS)
def test_flat_levels_of_mixed_modes_equal_the_contract(gpu, w, h, fmt):
    decode_case(f"mixed:{w}x{h}x1", fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", ["416x416x6", "420x420x6", "2048x514x1"])
def test_levels_around_the_block_per_lane_threshold_equal_the_contract(gpu, shape, fmt):
    """from 65536 blocks on a level whose width is a multiple of 4 goes to the block-per-lane kernel: 416^2 x 6 = 64896 blocks stay
    with the row-per-lane kernel, 420^2 x 6 = 66150 do not (105 blocks per row: a ragged second wave); 2048 x 514 = 66048 blocks with
    two of the last block row's four rows outside the level"""
    decode_case("mixed:" + shape, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("mode", D.MODE_VALUES)
def test_levels_of_one_mode_equal_the_contract(gpu, mode, fmt):
    """a 20^2 cube of one mode value throughout (wave-uniform control flow), for the 14 modes and the four reserved values (zeros)"""
    name = f"mode:{mode}"
    decode_case(name, fmt)
    if mode in D.RESERVED:
        assert not want_of(name, "f16")[..., :3].any()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", ["20x20x6", "7x9x1", "68x68x6"])
def test_the_encoders_own_output_decodes_as_the_contract(gpu, shape, fmt):
    name = "enc:" + shape
    b, w, h, layers = blocks_of(name)
    decode_case(name, fmt)
    if fmt == "f32":                                                          # and as the encoder-side decoder of mode 3 sees it
        assert np.array_equal(want_of(name, "f32").view(np.float32)[..., :3], R.decode_level(b, w, h, layers))


def make_chain(fmt, n=20, layers=6):
    import pbrhip
    flags = (pbrhip.TextureFlag_Cubemap if layers == 6 else 0) | pbrhip.TextureFlag_HasMipmaps
    return pbrhip.make_texture(gpu_format(fmt), n, n, flags)


def staged(L, blocks, pad=0, tail=0):
    """a mapped buffer holding `pad` bytes of 0xA5, the blocks, `tail` bytes of 0xA5"""
    import pbrhip
    raw = b"\xa5" * pad + np.ascontiguousarray(blocks).tobytes() + b"\xa5" * tail
    return L.GPU_MakeBuffer(len(raw), pbrhip.BufferFlag_CPU, raw)


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_into_one_level_leaves_the_others_untouched(gpu, fmt):
    """mip 1 of a 20^2 cube with the chain 20, 10, 5, ...: the bytes of mips 0 and 2 stay as they were; the blocks sit at offset 48"""
    import pbrhip
    L = gpu
    tex = make_chain(fmt)
    b, w, h, layers = blocks_of("mixed:10x10x6")
    dt = np.float32 if fmt == "f32" else np.uint16
    fill0 = np.full((6, 20, 20, 4), 3.0 if fmt == "f32" else 0x4200, dt)
    fill2 = np.full((6, 5, 5, 4), 5.0 if fmt == "f32" else 0x4500, dt)
    buf = staged(L, b, pad=48)
    g = L.GPU_MakeGraph()
    try:
        assert tex.contents.mip_level_count >= 3
        pbrhip.upload_mip(tex, 0, fill0); pbrhip.upload_mip(tex, 2, fill2)
        L.GPUX_OpDecodeBC6H(g, buf, 48, tex, 1)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        assert_level("mip 1", pbrhip.read_mip(tex, 1), want_of("mixed:10x10x6", fmt))
        assert pbrhip.read_mip_bytes(tex, 0) == fill0.tobytes() and pbrhip.read_mip_bytes(tex, 2) == fill2.tobytes()
    finally:
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(buf); L.GPU_DestroyTexture(tex)


def test_decode_of_blocks_encoded_in_the_same_graph(gpu):
    """GPUX_OpEncodeBC6H into a device buffer, GPUX_OpDecodeBC6H from it, one graph: ordered like any two ops"""
    import pbrhip
    L = gpu
    lvl = R.hdr_level(12, 12, 6, 1212)
    src = pbrhip.make_texture(pbrhip.Format_RGBA32F, 12, 12, pbrhip.TextureFlag_Cubemap, lvl)
    dst = pbrhip.make_texture(pbrhip.Format_RGBA32F, 12, 12, pbrhip.TextureFlag_Cubemap)
    dev = L.GPU_MakeBuffer(R.level_bytes(12, 12, 6), pbrhip.BufferFlag_GPU, None)
    g = L.GPU_MakeGraph()
    try:
        L.GPUX_OpEncodeBC6H(g, src, 0, dev, 0)
        L.GPUX_OpDecodeBC6H(g, dev, 0, dst, 0)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        got = pbrhip.read_mip(dst, 0)
        assert np.array_equal(got[..., :3], R.decode_level(R.encode(lvl), 12, 12, 6)) and (got[..., 3] == 1.0).all()
    finally:
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(dev); L.GPU_DestroyTexture(src); L.GPU_DestroyTexture(dst)


def test_graph_replay_gives_the_same_bytes(gpu):
    """the op is captured under GPUX_SetGraphReplay(1); instantiation and the updated replay give the plain bytes"""
    import pbrhip
    L = gpu
    b, w, h, layers = blocks_of("mixed:68x68x6")
    tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 68, 68, pbrhip.TextureFlag_Cubemap)
    buf = staged(L, b)
    results = []
    try:
        for replay in (0, 1):
            L.GPUX_SetGraphReplay(replay)
            g = L.GPU_MakeGraph()
            for _ in range(2):
                pbrhip.upload_mip(tex, 0, np.zeros((6, 68, 68, 4), np.float32))
                L.GPUX_OpDecodeBC6H(g, buf, 0, tex, 0)
                L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
                results.append(pbrhip.read_mip(tex, 0))
            s = [C.c_uint64() for _ in range(3)]
            L.GPUX_GraphReplayStats(g, *[C.byref(v) for v in s])
            print(f"replay {replay}: launches {s[0].value}, updates {s[1].value}, instantiations {s[2].value}")
            assert s[0].value == (2 if replay else 0)
            L.GPU_DestroyGraph(g)
    finally:
        L.GPUX_SetGraphReplay(-1)
        L.GPU_DestroyBuffer(buf); L.GPU_DestroyTexture(tex)
    for r in results:
        assert_level("under replay", r, want_of("mixed:68x68x6", "f32"))


def test_op_refuses_bad_arguments(gpu):
    """with an error handler installed a refused record reports and records nothing: only the accepted op of the graph runs"""
    import pbrhip
    L = gpu
    messages = []
    handler = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)(lambda msg, user: messages.append(msg.decode()))
    b, w, h, layers = blocks_of("mixed:4x4x6")                                 # 96 bytes
    tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 4, 4, pbrhip.TextureFlag_Cubemap)
    lut = pbrhip.make_texture(pbrhip.Format_RG16F, 4, 4, 0, np.zeros((4, 4, 2), np.float16))
    vol = pbrhip.make_texture(pbrhip.Format_RGBA16F, 4, 4, pbrhip.TextureFlag_StorageImage, depth=4)
    buf = staged(L, b, pad=160)                                               # 256 bytes
    g = L.GPU_MakeGraph()
    L.GPUX_SetErrorHandler(C.cast(handler, C.c_void_p), None)
    try:
        L.GPUX_OpDecodeBC6H(g, buf, 160, tex, 0)        # accepted: the last place where the 96 bytes are
        L.GPUX_OpDecodeBC6H(g, buf, 0, tex, 3)          # a mip past the chain
        L.GPUX_OpDecodeBC6H(g, buf, 8, tex, 0)          # offset not a multiple of 16
        L.GPUX_OpDecodeBC6H(g, buf, 176, tex, 0)        # 96 bytes are not there behind 176
        L.GPUX_OpDecodeBC6H(g, buf, 0, lut, 0)          # RG16F
        L.GPUX_OpDecodeBC6H(g, buf, 0, vol, 0)          # 3-D
        L.GPUX_OpDecodeBC6H(g, None, 0, tex, 0)
        L.GPUX_OpDecodeBC6H(g, buf, 0, None, 0)
        assert len(messages) == 7 and all("GPUX_OpDecodeBC6H" in m for m in messages), messages
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        assert_level("accepted", pbrhip.read_mip(tex, 0), want_of("mixed:4x4x6", "f32"))     # no refused record ran behind it (0xA5 padding, other offsets)
        assert not pbrhip.read_mip(lut, 0).any() and not pbrhip.read_mip(vol, 0).any()
        assert len(messages) == 7
    finally:
        L.GPUX_SetErrorHandler(None, None)
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(buf)
        for t in (tex, lut, vol):
            L.GPU_DestroyTexture(t)


def test_kernel_entry_point_checks_its_arguments(gpu):
    """pbrk_bc6h_decode returns an error and launches nothing for a null pointer, an extent of 0 or above 16384, no layers, another
    format, a misaligned pointer; the valid call afterwards writes the contract's bytes"""
    import pbrhip
    L = gpu
    OK, E_ARG, E_FORMAT = 0, -1, -2
    F32, F16, RG16F = 4, 3, 1                                                  # PBRK_FMT_*
    b, w, h, layers = blocks_of("mixed:5x5x6")
    nbytes = 6 * 5 * 5 * 8
    src_buf = staged(L, b)
    out = L.GPU_MakeBuffer(nbytes + 16, pbrhip.BufferFlag_CPU, None)
    try:
        src, dst = L.GPUX_BufferDevicePtr(src_buf), L.GPUX_BufferDevicePtr(out)
        C.memset(out.contents.data, 0x3C, nbytes + 16)
        bad = [((None, 5, 5, 6, dst, F16), E_ARG), ((src, 5, 5, 6, None, F16), E_ARG), ((src, 0, 5, 6, dst, F16), E_ARG), ((src, 5, 0, 6, dst, F16), E_ARG),
               ((src, 16385, 5, 6, dst, F16), E_ARG), ((src, 5, 16385, 6, dst, F16), E_ARG), ((src, 5, 5, 0, dst, F16), E_ARG), ((src, 5, 5, 65536, dst, F16), E_ARG),
               ((src, -5, 5, 6, dst, F16), E_ARG), ((src, 5, 5, 6, dst, RG16F), E_FORMAT), ((src, 5, 5, 6, dst, 0), E_FORMAT), ((src, 5, 5, 6, dst, 99), E_FORMAT),
               ((src + 8, 5, 5, 6, dst, F16), E_ARG), ((src, 5, 5, 6, dst + 8, F32), E_ARG), ((src, 5, 5, 6, dst + 4, F16), E_ARG)]
        for args, want in bad:
            assert L.pbrk_bc6h_decode(*args, None) == want, args
        L.GPU_WaitUntilIdle()
        assert C.string_at(out.contents.data, nbytes + 16) == b"\x3c" * (nbytes + 16)          # nothing was launched
        assert L.pbrk_bc6h_decode(src, 5, 5, 6, dst + 8, F16, None) == OK                       # an 8-byte aligned RGBA16F level: the narrow path
        L.GPU_WaitUntilIdle()
        raw = C.string_at(out.contents.data, nbytes + 16)
        assert raw[:8] == b"\x3c" * 8 and raw[8 + nbytes:] == b"\x3c" * 8
        assert_level("entry point", np.frombuffer(raw[8:8 + nbytes], np.uint16).reshape(6, 5, 5, 4), want_of("mixed:5x5x6", "f16"))
    finally:
        L.GPU_DestroyBuffer(out); L.GPU_DestroyBuffer(src_buf)


# ---- loader ----
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


def file_levels(data):
    """a BC6H .dds file -> (info, [blocks of level m, layer after layer])"""
    import pbrhip
    info = pbrhip.parse_dds_ex(data)
    assert info.dxgi_format == 95
    levels = []
    for m in range(info.level_count):
        per = info.level_size[m]
        levels.append(np.frombuffer(b"".join(data[info.level_offset[l][m]:info.level_offset[l][m] + per] for l in range(info.layers)), np.uint8).reshape(-1, 16))
    return info, levels


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("held", [2, 0])
def test_bc6h_dds_of_the_specular_cube_loads_back(gpu, bake, tmp_path, held, fmt):
    """the specular cube written as a BC6H file with a partial chain (16, 8) and with the whole chain (16 .. 1), loaded into either
    target format: every held level is the contract's decode of the file's blocks, the others are zero; the same with the level
    overlap of the scheduler off and on"""
    import pbrhip
    L = gpu
    tex = bake.tex_specular_env_map
    chain = tex.contents.mip_level_count
    assert chain == 5
    path = str(tmp_path / f"specular_{held}.dds")
    pbrhip.write_dds(path, tex, 0, held, pbrhip.PBR_DDS_OUT_BC6H_UF16)
    info, levels = file_levels(open(path, "rb").read())
    assert info.level_count == (held or chain) and (info.width, info.height, info.layers) == (16, 16, 6)
    loaded = []
    try:
        for overlap in (0, 1):
            L.GPUX_SetLevelOverlap(overlap)
            back = pbrhip.make_texture_from_bc6h_dds_file(path, gpu_format(fmt))
            b = back.contents
            assert (b.format, b.width, b.height, b.layer_count, b.mip_level_count) == (gpu_format(fmt), 16, 16, 6, chain)
            got = [pbrhip.read_mip(back, m) for m in range(chain)]
            L.GPU_DestroyTexture(back)
            for m in range(chain):
                n = 16 >> m
                if m < info.level_count:
                    want = D.level_rgba(levels[m], n, n, 6, fmt == "f32")
                    assert_level(f"level {m}, overlap {overlap}", got[m], bits(want))
                else:
                    assert not bits(got[m]).any(), (m, overlap)
            loaded.append(b"".join(bits(a).tobytes() for a in got))
    finally:
        L.GPUX_SetLevelOverlap(1)
    assert loaded[0] == loaded[1]
    for m in range(info.level_count):                                         # the file holds what K18 wrote: mode 3, near the source
        assert (D.modes_of(levels[m]) == 3).all()


def test_one_level_2d_file_and_the_refusals_of_the_loader(gpu, tmp_path):
    """a flat 20 x 12 file of mixed modes (a foreign file) gives a texture without mips; a float file, a truncated file, another target
    format and a missing file give no texture"""
    import pbrhip
    L = gpu
    b, w, h, layers = blocks_of("mixed:20x12x1")
    head = (C.c_uint8 * 148)()
    total = L.PBR_BuildDDSHeader(95, 20, 12, 1, 1, head, None)
    data = bytes(head) + b.tobytes()
    assert total == len(data)
    path = str(tmp_path / "flat.dds")
    open(path, "wb").write(data)
    t = pbrhip.make_texture_from_bc6h_dds_file(path, pbrhip.Format_RGBA16F)
    try:
        c = t.contents
        assert (c.format, c.width, c.height, c.layer_count, c.mip_level_count) == (pbrhip.Format_RGBA16F, 20, 12, 1, 1)
        assert_level("flat file", pbrhip.read_mip(t, 0)[None], want_of("mixed:20x12x1", "f16"))
    finally:
        L.GPU_DestroyTexture(t)
    assert not L.PBR_MakeTextureFromBC6HDDSMemory(data, len(data) - 1, pbrhip.Format_RGBA16F)
    assert not L.PBR_MakeTextureFromBC6HDDSMemory(data, len(data), pbrhip.Format_RG16F)
    L.PBR_BuildDDSHeader(10, 20, 12, 1, 1, head, None)
    flt = bytes(head) + bytes(20 * 12 * 8)
    assert not L.PBR_MakeTextureFromBC6HDDSMemory(flt, len(flt), pbrhip.Format_RGBA16F)
    with pytest.raises(RuntimeError):
        pbrhip.make_texture_from_bc6h_dds_file(str(tmp_path / "missing.dds"), pbrhip.Format_RGBA32F)


# ---- lighting ----
def test_lighting_after_a_decode_into_the_bound_specular_cube(gpu):
    """a frame lit with one specular cube (its sampler twins are built), then level 0 of that cube overwritten by GPUX_OpDecodeBC6H and
    the frame lit again: equal to the frame lit from a fresh texture uploaded with the same decoded bytes -- the op dropped the twins"""
    import gpu_rigs
    import shade_maps as M
    L = gpu
    case = M.ShadeCase(33, 9, 16, 8, 16)
    blocks = R.encode(M.cube_level(16, 0, variant=2))
    decoded = D.level_rgba(blocks, 16, 16, 6, True)
    rig = gpu_rigs.ShadeRig(L, case)
    buf = staged(L, blocks)
    try:
        before = rig.draw_api(M.IBL)
        L.GPUX_OpDecodeBC6H(rig.g, buf, 0, rig.maps.tex_specular_env_map, 0)
        L.GPU_GraphSubmit(rig.g); L.GPU_GraphWait(rig.g)
        after = rig.draw_api(M.IBL)
    finally:
        L.GPU_DestroyBuffer(buf); rig.destroy()
    case.pre_levels[0] = decoded
    fresh_rig = gpu_rigs.ShadeRig(L, case)
    try:
        fresh = fresh_rig.draw_api(M.IBL)
    finally:
        fresh_rig.destroy()
    assert after.tobytes() == fresh.tobytes()
    assert before.tobytes() != after.tobytes()                                # and level 0 is sampled by this frame


# ---- pbr_demo ----
def test_demo_shades_from_the_files_it_saved(gpu, tmp_path):
    """pbr_demo ... dds P, then pbr_demo ... ddsin P: the second run bakes nothing, loads the three files (the specular cube through
    K19) and goes on; the float maps give the first run's sums, the held specular levels are printed"""
    import pbrhip
    from pbrhip import synth
    hdr = tmp_path / "cube_strip.hdr"
    hdr.write_bytes(synth.env_to_hdr_strip(synth.synth_env(64, seed=0x5EED0018), rle=True))
    exe = os.path.join(pbrhip.PKG_ROOT, "pbr_demo")
    sizes = ["32", "256", "64", "16", "320", "180"]
    prefix = str(tmp_path / "bake")

    def lines(extra):
        out = subprocess.run([exe, str(hdr), *sizes, *extra], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if not l.startswith(("time_ms", "dds_bytes"))}, out.stdout.splitlines()

    first, _ = lines(["dds", prefix])
    second, raw = lines(["ddsin", prefix])
    assert raw[-1] == "ok 1"
    assert second["irradiance_sum"] == first["irradiance_sum"] and second["lut_bits_sum"] == first["lut_bits_sum"]
    assert list(second) == list(first)                                        # the same lines in the same order
    for m in range(3):                                                        # 64, 32, 16: the levels the file holds (BC6H is lossy: other sums)
        assert np.isfinite(float(second[f"specular_mip{m}_sum"][0])) and float(second[f"specular_mip{m}_sum"][0]) > 0.0
    assert "specular_mip3_sum" not in second
