"""K20 on the GPU: one level of an RGBA32F cube as a lat-long panorama, held bit for bit to the numpy restatement of the sampler
(tests/panorama_ref.py) fed with the directions the library itself reports -- through the graph op, the host layer, hipGraph replay
and pbr_demo.  The largest panorama is 256 x 128."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panorama_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cube_of(gpu):
    """n -> (texture with the generated chain, {mip: the level as the GPU holds it}); made once, shared, never written by a test"""
    import pbrhip
    made = {}

    def get(n):
        if n not in made:
            tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, n, n, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, P.hdr_cube(n, 0x20C0 + n))
            levels = {}
            for m in range(tex.contents.mip_level_count):
                levels[m] = pbrhip.read_mip(tex, m)
                levels[m].setflags(write=False)
            made[n] = (tex, levels)
        return made[n]

    yield get
    for tex, _ in made.values():
        gpu.GPU_DestroyTexture(tex)


def fresh_cube(n, data):
    import pbrhip
    return pbrhip.make_texture(pbrhip.Format_RGBA32F, n, n, pbrhip.TextureFlag_Cubemap, np.ascontiguousarray(data, np.float32))


def run(L, g):
    L.GPU_GraphSubmit(g)
    L.GPU_GraphWait(g)


def panorama_into(L, cube, src_mip, dst, dst_mip=0):
    g = L.GPU_MakeGraph()
    L.GPUX_OpCubeToPanorama(g, cube, src_mip, dst, dst_mip)
    run(L, g)
    L.GPU_DestroyGraph(g)


def panorama_of(L, cube, src_mip, w, h, fmt=None):
    import pbrhip
    dst = pbrhip.make_texture(pbrhip.Format_RGBA32F if fmt is None else fmt, w, h, 0)
    try:
        panorama_into(L, cube, src_mip, dst)
        return pbrhip.read_mip(dst, 0)
    finally:
        L.GPU_DestroyTexture(dst)


def assert_bits(label, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    ib = np.uint32 if got.dtype == np.float32 else np.uint16
    bad = np.argwhere(got.view(ib) != want.view(ib))
    assert len(bad) == 0, (label, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# (cube, source mip, w, h): what each can break
EXACT = [(8, 0, 32, 16),       # w = 4 n: the phi = pi / 4 face ties
         (8, 3, 7, 5),         # n = 1: every tap is apron or corner
         (8, 2, 37, 19),       # n = 2, ragged in both axes
         (12, 2, 64, 32),      # n = 3: a level that is no power of two; exactly one full wave
         (8, 0, 130, 3),       # three column blocks, the last of two lanes; fewer rows than a workgroup
         (8, 0, 1, 1), (8, 0, 5, 1),
         (64, 0, 256, 128)]    # many workgroups


@pytest.mark.parametrize("n,mip,w,h", EXACT)
def test_panorama_equals_the_restatement_bit_for_bit(gpu, cube_of, n, mip, w, h):
    tex, levels = cube_of(n)
    assert levels[mip].shape[1] == max(1, n >> mip)
    assert_bits(f"cube {n} mip {mip} {w}x{h}", panorama_of(gpu, tex, mip, w, h), P.panorama(levels[mip], w, h))


def test_half_target_equals_the_rounded_restatement(gpu, cube_of):
    """33 x 17: the 8-byte stores of odd pixels are not 16-byte aligned; fp16 by round to nearest even, as numpy's astype"""
    import pbrhip
    tex, levels = cube_of(8)
    got = panorama_of(gpu, tex, 0, 33, 17, pbrhip.Format_RGBA16F)
    assert_bits("f16 33x17", got, P.panorama(levels[0], 33, 17).astype(np.float16))


def test_target_level_two_is_written_and_the_others_are_not(gpu, cube_of):
    import pbrhip
    L = gpu
    tex, levels = cube_of(8)
    dst = pbrhip.make_texture(pbrhip.Format_RGBA32F, 64, 32, pbrhip.TextureFlag_HasMipmaps)
    try:
        count = dst.contents.mip_level_count
        assert count >= 4
        for m in range(count):
            pbrhip.upload_mip(dst, m, np.full((max(1, 32 >> m), max(1, 64 >> m), 4), -7.0 - m, np.float32))
        panorama_into(L, tex, 0, dst, 2)
        assert_bits("dst mip 2", pbrhip.read_mip(dst, 2), P.panorama(levels[0], 16, 8))
        for m in range(count):
            if m != 2:
                assert (pbrhip.read_mip(dst, m) == np.float32(-7.0 - m)).all(), m
    finally:
        L.GPU_DestroyTexture(dst)


def test_hostile_texels(gpu):
    """one +inf, one NaN, negative values and 1e30: pixels whose four taps are finite are bit-identical, the others are the same set"""
    L = gpu
    rng = np.random.default_rng(0x20C1)
    lvl = rng.normal(0.0, 3.0, (6, 8, 8, 4)).astype(np.float32)
    lvl[0, 3, 4, 0] = np.inf
    lvl[2, 0, 7, 1] = np.nan                                                  # on an edge: in two aprons
    lvl[4, 5, 5, :] = np.float32(1e30)
    lvl[5, 0, 0, 2] = np.float32(-1e30)                                       # a corner texel: in three corner means
    cube = fresh_cube(8, lvl)
    try:
        got = panorama_of(L, cube, 0, 32, 16)
    finally:
        L.GPU_DestroyTexture(cube)
    import pbrhip
    want, taps = P.sample(lvl, pbrhip.panorama_directions(32, 16), with_taps=True)
    finite = np.isfinite(taps).all(axis=0)
    assert finite.mean() > 0.8 and not finite.all()
    assert (got.view(np.uint32)[finite] == want.view(np.uint32)[finite]).all()
    assert (np.isfinite(got) == np.isfinite(want)).all()


@pytest.mark.parametrize("n", [4, 16])
def test_orientation_with_one_colour_per_face(gpu, n):
    """independent of any sampler: where the fp64 direction's second-largest component is at most (1 - 2 / n) of the largest, all four
    taps lie inside the face the direction points at, and a lerp of equal values is that value exactly"""
    L = gpu
    colours = np.array([[f + 1, 10 * (f + 1), 100 * (f + 1), 1] for f in range(6)], np.float32)
    cube = fresh_cube(n, np.broadcast_to(colours[:, None, None, :], (6, n, n, 4)))
    try:
        got = panorama_of(L, cube, 0, 48, 24)
    finally:
        L.GPU_DestroyTexture(cube)
    d = P.directions_f64(48, 24)
    mag = np.sort(np.abs(d), axis=-1)
    inside = mag[..., 1] <= (1 - 2.0 / n) * mag[..., 2]
    axis = np.argmax(np.abs(d), axis=-1)
    face = 2 * axis + (np.take_along_axis(d, axis[..., None], -1)[..., 0] < 0)
    for f in range(6):
        sel = inside & (face == f)
        assert sel.sum() >= 52, (f, int(sel.sum()))
        assert (got[sel] == colours[f]).all(), f
    print(f"n {n}: {float(inside.mean()):.2f} of the pixels qualify")


@pytest.mark.parametrize("cx,cy", [(0, 16), (63, 10), (20, 5), (40, 27)])
def test_round_trip_through_the_equirect_loader(gpu, cx, cy):
    """a 3 x 3 block with a bright centre -> K6 (face 32) -> K20 at the same extent: the maximum comes back within one pixel; x wraps"""
    L = gpu
    w, h = 64, 32
    eq = np.full((h, w, 4), 0.01, np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            eq[min(max(cy + dy, 0), h - 1), (cx + dx) % w, :3] = 50.0
    eq[cy, cx, :3] = 100.0
    cube = L.GPUX_MakeCubemapFromEquirect(eq.ctypes.data_as(C.c_void_p), w, h, 32, 0)
    assert cube
    try:
        got = panorama_of(L, cube, 0, w, h)
    finally:
        L.GPU_DestroyTexture(cube)
    y, x = np.unravel_index(int(np.argmax(got[..., 0])), (h, w))
    dx = min((x - cx) % w, (cx - x) % w)
    assert dx <= 1 and abs(int(y) - cy) <= 1, (x, y)


def test_effects_are_followed(gpu):
    """the apron K20 samples is rebuilt after a write to the cube -- between two submissions of one graph (GPU_GraphWait resets a graph,
    so the op is recorded again on it), and between two ops of one submission; the apron build is a timed entry of its own; a target
    that was read before shows the new bytes on the next read"""
    import pbrhip
    L = gpu
    old, new = P.hdr_cube(8, 0x20C2), P.hdr_cube(8, 0x20C3)
    want_old, want_new = P.panorama(old, 24, 12), P.panorama(new, 24, 12)
    cube = fresh_cube(8, old)
    dst = pbrhip.make_texture(pbrhip.Format_RGBA32F, 24, 12, 0)
    dst2 = pbrhip.make_texture(pbrhip.Format_RGBA32F, 24, 12, 0)
    staging = L.GPU_MakeBuffer(new.nbytes, pbrhip.BufferFlag_CPU, new.ctypes.data_as(C.c_void_p))
    g = L.GPU_MakeGraph()
    L.GPUX_EnableOpTiming(1)
    try:
        names = []
        for k, want in enumerate((want_old, want_new, want_new)):
            L.GPUX_OpCubeToPanorama(g, cube, 0, dst, 0)
            run(L, g)
            names.append([L.GPUX_GraphTimedOpName(g, i).decode() for i in range(L.GPUX_GraphTimedOpCount(g))])
            assert_bits(f"submission {k}", pbrhip.read_mip(dst, 0), want)
            if k == 0:
                pbrhip.upload_mip(cube, 0, new)                               # a writer of the cube, on another graph
        assert names == [["apron.panorama", "K20.cube_to_panorama"]] * 2 + [["K20.cube_to_panorama"]], names
        # one submission: panorama of the new data, the old data copied back onto the cube, panorama of that
        pbrhip.upload_mip(cube, 0, new)
        C.memmove(staging.contents.data, old.ctypes.data, old.nbytes)
        L.GPUX_OpCubeToPanorama(g, cube, 0, dst, 0)
        L.GPUX_OpCopyBufferToTextureMip(g, staging, 0, cube, 0)
        L.GPUX_OpCubeToPanorama(g, cube, 0, dst2, 0)
        run(L, g)
        assert_bits("in front of the copy", pbrhip.read_mip(dst, 0), want_new)
        assert_bits("behind the copy", pbrhip.read_mip(dst2, 0), want_old)
    finally:
        L.GPUX_EnableOpTiming(0)
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(staging)
        for t in (cube, dst, dst2):
            L.GPU_DestroyTexture(t)


def test_host_layer(gpu, cube_of, tmp_path):
    import pbrhip
    L = gpu
    tex, levels = cube_of(12)
    floats = pbrhip.cube_to_panorama(tex, 1)                                  # n = 6: the default extent
    assert floats.shape == (12, 24, 4) and floats.dtype == np.float32
    assert_bits("default extent", floats, P.panorama(levels[1], 24, 12))
    halves = pbrhip.cube_to_panorama(tex, 1, 10, 0, pbrhip.Format_RGBA16F)
    assert halves.dtype == np.uint16
    assert_bits("half, height 0", halves, P.panorama(levels[1], 10, 5).astype(np.float16).view(np.uint16))
    # .hdr: byte-identical to the RGBE encoding of the floats
    path = tmp_path / "pano.hdr"
    assert L.PBR_WritePanoramaHDR(os.fsencode(str(path)), tex, 1, 0, 0) == 0
    size = C.c_size_t(0)
    p = L.PBR_EncodeHDR(floats.ctypes.data_as(C.c_void_p), 24, 12, C.byref(size))
    assert p
    try:
        assert path.read_bytes() == C.string_at(p, size.value)
    finally:
        pbrhip._libc_free(p)
    assert b"-Y 12 +X 24\n" in path.read_bytes()[:80]
    # .dds: nothing new, PBR_WriteTextureDDS of the texture
    pano = L.PBR_MakePanoramaFromCube(tex, 1, 0, 0, pbrhip.Format_RGBA32F)
    assert pano and (pano.contents.width, pano.contents.height, pano.contents.layer_count) == (24, 12, 1)
    try:
        dds = tmp_path / "pano.dds"
        pbrhip.write_dds(str(dds), pano)
    finally:
        L.GPU_DestroyTexture(pano)
    data = dds.read_bytes()
    info = pbrhip.parse_dds_ex(data)
    assert (info.dxgi_format, info.width, info.height, info.layers, info.level_count) == (2, 24, 12, 1, 1)
    off = info.level_offset[0][0]
    assert info.level_size[0] == floats.nbytes and data[off:off + floats.nbytes] == floats.tobytes()
    # errors give NULL / non-zero
    lut = pbrhip.make_texture(pbrhip.Format_RG16F, 4, 4, 0)
    try:
        assert not L.PBR_MakePanoramaFromCube(lut, 0, 0, 0, pbrhip.Format_RGBA32F)
        assert not L.PBR_MakePanoramaFromCube(tex, 9, 0, 0, pbrhip.Format_RGBA32F)
        assert not L.PBR_MakePanoramaFromCube(tex, 0, 0, 0, pbrhip.Format_RG16F)
        assert not L.PBR_MakePanoramaFromCube(tex, 0, 16385, 1, pbrhip.Format_RGBA32F)
        assert L.PBR_WritePanoramaHDR(os.fsencode(str(tmp_path / "none.hdr")), None, 0, 0, 0) != 0
    finally:
        L.GPU_DestroyTexture(lut)


def test_bad_arguments_are_one_error_each_and_record_nothing(gpu, cube_of):
    import pbrhip
    L = gpu
    messages = []
    handler = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)(lambda msg, user: messages.append(msg.decode()))
    tex, _ = cube_of(8)
    sentinel = np.full((4, 8, 4), -3.0, np.float32)
    dst = pbrhip.make_texture(pbrhip.Format_RGBA32F, 8, 4, 0, sentinel)
    half_cube = pbrhip.make_texture(pbrhip.Format_RGBA16F, 4, 4, pbrhip.TextureFlag_Cubemap)
    flat = pbrhip.make_texture(pbrhip.Format_RGBA32F, 4, 4, 0)
    lut = pbrhip.make_texture(pbrhip.Format_RG16F, 4, 4, 0)
    cube_dst = pbrhip.make_texture(pbrhip.Format_RGBA32F, 4, 4, pbrhip.TextureFlag_Cubemap)
    vol = pbrhip.make_texture(pbrhip.Format_RGBA16F, 4, 4, pbrhip.TextureFlag_StorageImage, depth=4)
    wide = pbrhip.make_texture(pbrhip.Format_RGBA16F, 16385, 1, 0)
    tall = pbrhip.make_texture(pbrhip.Format_RGBA16F, 1, 16385, 0)
    sun = L.PBR_MakeSunDepthPass(64)
    g = L.GPU_MakeGraph()
    L.GPUX_SetErrorHandler(C.cast(handler, C.c_void_p), None)
    L.GPUX_EnableOpTiming(1)
    try:
        bad = [(None, 0, dst, 0), (tex, 0, None, 0),                          # NULL
               (half_cube, 0, dst, 0), (flat, 0, dst, 0),                     # the source: an RGBA16F cube, a 2-D texture
               (tex, 0, lut, 0), (tex, 0, cube_dst, 0), (tex, 0, vol, 0),     # the target: another format, a cube, 3-D
               (tex, 4, dst, 0), (tex, 0, dst, 1),                            # a mip past either chain
               (tex, 0, wide, 0), (tex, 0, tall, 0)]                          # an extent above 16384
        for k, args in enumerate(bad):
            L.GPUX_OpCubeToPanorama(g, *args)
            assert len(messages) == k + 1, (k, messages)
        L.GPU_OpPrepareRenderPass(g, L.PBR_SunDepthRenderPass(sun))
        L.GPU_OpBeginRenderPass(g)
        L.GPUX_OpCubeToPanorama(g, tex, 0, dst, 0)                            # inside a render pass
        L.GPU_OpEndRenderPass(g)
        assert len(messages) == len(bad) + 1 and "inside a render pass" in messages[-1], messages
        run(L, g)
        assert L.GPUX_GraphTimedOpCount(g) == 0                              # nothing was recorded
        assert (pbrhip.read_mip(dst, 0) == sentinel).all()
        assert all(m.startswith("GPUX_OpCubeToPanorama: ") for m in messages), messages
    finally:
        L.GPUX_EnableOpTiming(0)
        L.GPUX_SetErrorHandler(None, None)
        L.GPU_DestroyGraph(g)
        L.PBR_DestroySunDepthPass(sun)
        for t in (dst, half_cube, flat, lut, cube_dst, vol, wide, tall):
            L.GPU_DestroyTexture(t)


def test_graph_replay_leaves_the_op_on_the_plain_path(gpu, cube_of):
    """a graph that holds the op is not captured under GPUX_SetGraphReplay(1) and gives the same bytes"""
    import pbrhip
    L = gpu
    tex, levels = cube_of(8)
    want = P.panorama(levels[0], 40, 20)
    dst = pbrhip.make_texture(pbrhip.Format_RGBA32F, 40, 20, 0)
    g = L.GPU_MakeGraph()
    try:
        L.GPUX_SetGraphReplay(1)
        for _ in range(2):
            pbrhip.upload_mip(dst, 0, np.zeros((20, 40, 4), np.float32))
            L.GPUX_OpCubeToPanorama(g, tex, 0, dst, 0)
            run(L, g)
            assert_bits("under replay", pbrhip.read_mip(dst, 0), want)
        s = [C.c_uint64(0) for _ in range(3)]
        L.GPUX_GraphReplayStats(g, *[C.byref(v) for v in s])
        assert [v.value for v in s] == [0, 0, 0]
    finally:
        L.GPUX_SetGraphReplay(-1)
        L.GPU_DestroyGraph(g); L.GPU_DestroyTexture(dst)


def test_demo_writes_one_panorama_per_level(gpu, tmp_path):
    """pbr_demo ... pano P: P_irradiance.hdr and P_specular_mipN.hdr for the levels the bake wrote, at 4 n x 2 n; the other lines stay"""
    import pbrhip
    from pbrhip import synth
    hdr = tmp_path / "cube_strip.hdr"
    hdr.write_bytes(synth.env_to_hdr_strip(synth.synth_env(64, seed=0x5EED0020), rle=True))
    exe = os.path.join(pbrhip.PKG_ROOT, "pbr_demo")
    prefix = str(tmp_path / "bake")
    out = subprocess.run([exe, str(hdr), "16", "64", "32", "8", "64", "36", "pano", prefix], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok 1"
    want = {"irradiance": 16, "specular_mip0": 32, "specular_mip1": 16, "specular_mip2": 8}
    assert [l.split()[1:] for l in lines if l.startswith("pano_extent")] == [[k, str(4 * n), str(2 * n)] for k, n in want.items()]
    assert sorted(p.name for p in tmp_path.glob("bake_*.hdr")) == sorted(f"bake_{k}.hdr" for k in want)
    for k, n in want.items():
        head = (tmp_path / f"bake_{k}.hdr").read_bytes()[:80]
        assert head.startswith(b"#?RADIANCE\n") and f"-Y {2 * n} +X {4 * n}\n".encode() in head, (k, head)
