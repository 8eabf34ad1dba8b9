"""K17 on the GPU: SH9 projection of cube levels and the irradiance cube of nine coefficients against the numpy restatement
(tests/sh_ref.py), through the graph ops, the host layer and hipGraph replay.  Cubes are at most 96 x 96.

Projection tolerance: each coefficient within 1e-10 S[k][c] of the restatement, S = sum |L Y domega| over the same texels:
  * reordering N <= 6 * 96^2 = 55 296 fp64 terms costs at most N 2^-53 ~ 6e-12 of S;
  * domega is a difference of four atan2 values of magnitude <= 0.62, so an ulp of atan2 costs about 4 * 2^-53 * 0.62 / min domega
    ~ 1.4e-12 of a term at n = 64 (min domega ~ 2e-4), and the device's atan2 is allowed a few ulp;
  * 1e-10 leaves roughly tenfold margin over their sum.
Synthesis tolerance: |got - want| <= 2^-22 sum_k |a_k coef Y_k| per channel -- the one fp32 rounding (2^-24) with fourfold margin."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sh_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

PROJECT_TOL = 1e-10
SYNTH_TOL = 2.0 ** -22

_CUBES, _WANT = {}, {}


def cube_of(n):
    if n not in _CUBES:
        _CUBES[n] = R.hdr_cube(n, 100 + n)
        _CUBES[n].setflags(write=False)
    return _CUBES[n]


def want_of(n, faces=(0, 6), rows=None):
    key = (n, faces, rows)
    if key not in _WANT:
        _WANT[key] = R.project(cube_of(n), faces, rows)
    return _WANT[key]


def cube_texture(data, mips=False):
    import pbrhip
    n = data.shape[1]
    return pbrhip.make_texture(pbrhip.Format_RGBA32F, n, n, pbrhip.TextureFlag_Cubemap | (pbrhip.TextureFlag_HasMipmaps if mips else 0), data)


def empty_cube(size):
    import pbrhip
    return pbrhip.make_texture(pbrhip.Format_RGBA32F, size, size, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_StorageImage, None)


def check_projection(label, got, want, S):
    worst = R.worst_ratio(np.abs(got - want), S)
    print(f"{label}: worst {worst:.3g} / tolerance {PROJECT_TOL:g} of S")
    assert worst <= PROJECT_TOL, label


@pytest.mark.parametrize("n", [1, 3, 5, 64, 96])
def test_projection_equals_the_restatement(gpu, n):
    """1: one texel per face; 3, 5: odd, a wave's lanes end inside the tile; 64: several partials enter stage two; 96: not a power of
    two, a second column of tiles with half its lanes outside the level, many workgroups"""
    import pbrhip
    tex = cube_texture(cube_of(n))
    try:
        got = pbrhip.project_sh9(tex, 0)
        check_projection(f"n={n}", got, *want_of(n))
    finally:
        gpu.GPU_DestroyTexture(tex)


def test_projection_of_a_mip_level(gpu):
    """mip 2 of a 32^2 cube created with mips: the level's offset inside the pyramid"""
    import pbrhip
    tex = cube_texture(cube_of(32), mips=True)
    try:
        level = pbrhip.read_mip(tex, 2)
        assert level.shape == (6, 8, 8, 4)
        got = pbrhip.project_sh9(tex, 2)
        want, S = R.project(level)
        check_projection("32^2 mip 2", got, want, S)
        assert not np.array_equal(got, pbrhip.project_sh9(tex, 1))
    finally:
        gpu.GPU_DestroyTexture(tex)


def test_same_op_gives_the_same_bytes(gpu):
    """submitted twice, and twice inside one graph at two offsets of one buffer (they share the graph's scratch)"""
    import pbrhip
    L = gpu
    tex = cube_texture(cube_of(96))
    buf = L.GPU_MakeBuffer(3 * 216, pbrhip.BufferFlag_CPU, None)
    g = L.GPU_MakeGraph()
    try:
        runs = []
        for _ in range(2):
            C.memset(buf.contents.data, 0xFF, 3 * 216)
            L.GPUX_OpProjectSH9(g, tex, 0, 0, 6, 0, 96, buf, 0)
            L.GPUX_OpProjectSH9(g, tex, 0, 0, 6, 0, 96, buf, 432)
            L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
            raw = C.string_at(buf.contents.data, 3 * 216)
            assert raw[216:432] == b"\xff" * 216                                # only the 216 bytes at each offset are written
            runs += [raw[:216], raw[432:]]
        assert runs[0] == runs[1] == runs[2] == runs[3]
        assert runs[0] == pbrhip.project_sh9(tex, 0).tobytes()
    finally:
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(buf); L.GPU_DestroyTexture(tex)


def test_shards(gpu):
    """a sub-range gives that range's partial sum; a cover of the level by three ragged shards adds up to the whole"""
    import pbrhip
    n = 64
    tex = cube_texture(cube_of(n))
    try:
        got = pbrhip.project_sh9(tex, 0, faces=(1, 4), rows=(7, 29))
        check_projection("faces [1, 4) x rows [7, 29)", got, *want_of(n, (1, 4), (7, 29)))
        total = np.zeros((9, 3))
        for faces, rows in (((0, 2), (0, 64)), ((2, 6), (0, 23)), ((2, 6), (23, 64))):
            part = pbrhip.project_sh9(tex, 0, faces=faces, rows=rows)
            check_projection(f"faces {faces} x rows {rows}", part, *want_of(n, faces, rows))
            total += part
        check_projection("sum of three shards", total, *want_of(n))
    finally:
        gpu.GPU_DestroyTexture(tex)


@pytest.fixture(scope="module")
def coef16():
    c, _ = R.project(R.hdr_cube(16, 7))
    c.setflags(write=False)
    return c


@pytest.mark.parametrize("size", [1, 3, 32, 40])
def test_synthesis_equals_the_restatement(gpu, coef16, size):
    import pbrhip
    tex = empty_cube(size)
    try:
        pbrhip.irradiance_from_sh9(coef16, tex, 0)
        got = pbrhip.read_mip(tex, 0)
        want, bound = R.irradiance(coef16, size), R.irradiance_bound(coef16, size)
        worst = R.worst_ratio(np.abs(got[..., :3] - want), bound)
        print(f"synthesis size={size}: worst {worst:.3g} / tolerance {SYNTH_TOL:.3g} of sum |a c Y|; min {got[..., :3].min():.3g} (not clamped)")
        assert worst <= SYNTH_TOL
        assert not got[..., 3].view(np.uint32).any()
    finally:
        gpu.GPU_DestroyTexture(tex)


def test_synthesis_writes_only_the_level_it_names(gpu, coef16):
    import pbrhip
    tex = cube_texture(cube_of(32), mips=True)
    try:
        before = [pbrhip.read_mip(tex, m) for m in range(tex.contents.mip_level_count)]
        pbrhip.irradiance_from_sh9(coef16, tex, 1)
        for m, b in enumerate(before):
            got = pbrhip.read_mip(tex, m)
            if m == 1:
                bound = R.irradiance_bound(coef16, 16)
                assert R.worst_ratio(np.abs(got[..., :3] - R.irradiance(coef16, 16)), bound) <= SYNTH_TOL
            else:
                assert np.array_equal(got, b), m
    finally:
        gpu.GPU_DestroyTexture(tex)


def test_host_layer_equals_the_ops(gpu):
    import pbrhip
    L = gpu
    env = cube_texture(cube_of(32), mips=True)
    a, b = empty_cube(8), empty_cube(8)
    try:
        for mip in (0, 2):
            out = np.zeros(27)
            assert L.PBR_ProjectSH9(env, mip, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
            op = pbrhip.project_sh9(env, mip)
            assert out.tobytes() == op.tobytes()
            L.PBR_GenIrradianceMapSH(env, mip, a)
            pbrhip.irradiance_from_sh9(op, b, 0)
            assert pbrhip.read_mip(a, 0).tobytes() == pbrhip.read_mip(b, 0).tobytes()
        assert L.PBR_ProjectSH9(env, 99, np.zeros(27).ctypes.data_as(C.POINTER(C.c_double))) != 0
    finally:
        for t in (env, a, b):
            L.GPU_DestroyTexture(t)


def test_graph_replay_gives_the_same_bytes(gpu):
    """a graph holding both ops is captured under GPUX_SetGraphReplay(1); instantiation and the updated replay give the plain bytes"""
    import pbrhip
    L = gpu
    env = cube_texture(cube_of(64))
    irr = empty_cube(8)
    buf = L.GPU_MakeBuffer(216, pbrhip.BufferFlag_CPU, None)
    results = []
    try:
        for replay in (0, 1):
            L.GPUX_SetGraphReplay(replay)
            g = L.GPU_MakeGraph()
            for _ in range(2):
                C.memset(buf.contents.data, 0, 216)
                L.GPU_OpClearColorF(g, irr, 0, 9.0, 9.0, 9.0, 9.0)
                L.GPUX_OpProjectSH9(g, env, 0, 0, 6, 0, 64, buf, 0)
                L.GPUX_OpIrradianceFromSH9(g, buf, 0, irr, 0)
                L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
                results.append((C.string_at(buf.contents.data, 216), pbrhip.read_mip(irr, 0).tobytes()))
            s = [C.c_uint64() for _ in range(3)]
            L.GPUX_GraphReplayStats(g, *[C.byref(v) for v in s])
            print(f"replay {replay}: launches {s[0].value}, updates {s[1].value}, instantiations {s[2].value}")
            assert s[0].value == (2 if replay else 0)
            L.GPU_DestroyGraph(g)
    finally:
        L.GPUX_SetGraphReplay(-1)
        L.GPU_DestroyBuffer(buf); L.GPU_DestroyTexture(env); L.GPU_DestroyTexture(irr)
    assert all(r == results[0] for r in results)
    check_projection("under replay", np.frombuffer(results[3][0], np.float64).reshape(9, 3), *want_of(64))


def test_overwritten_irradiance_map_is_what_the_lighting_pass_samples(gpu):
    """the write op drops the target's sampler twins: a frame shaded after GPUX_OpIrradianceFromSH9 overwrote K3's map differs from
    the one before and is bit-identical to a fresh lighting pass over a cube uploaded with the same texels"""
    import pbrhip
    from pbrhip import synth
    L = gpu
    W, H = 64, 36
    env = synth.synth_env(64, seed=0x5EED00AA)
    env_tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 64, 64, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), 16, 64, 32)
    L.PBR_GenPrefilteredEnvMap(env_tex, maps.tex_specular_env_map, 1)
    L.PBR_GenIrradianceMap(env_tex, maps.irradiance_map)
    L.PBR_GenBRDFIntegrationMap(maps.brdf_lut)
    gbd = synth.synth_gbuffer_spheres(W, H)
    gb = pbrhip.PBR_GBuffer()
    L.PBR_MakeGBuffer(C.byref(gb), W, H, pbrhip.Format_RGBA32F)
    for name, arr in (("base_color", gbd["base"]), ("normal", gbd["normal"]), ("orm", gbd["orm"]), ("emissive", gbd["emissive"]), ("depth", gbd["depth"])):
        pbrhip.upload_mip(getattr(gb, name), 0, arr)
    glob = pbrhip.fill_globals(gbd["cam_pos"], aspect=W / H)

    def shade(lp):
        g = L.GPU_MakeGraph()
        L.PBR_RecordLightingPass(lp, g, C.byref(glob), 0, 0)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        L.GPU_DestroyGraph(g)
        return pbrhip.read_mip(gb.lighting_result, 0)

    lp = L.PBR_MakeLightingPass(C.byref(gb), C.byref(maps), W, H)
    first = shade(lp)
    pbrhip.irradiance_from_sh9(pbrhip.project_sh9(env_tex, 0), maps.irradiance_map, 0)
    second = shade(lp)
    assert not np.array_equal(first, second)
    texels = pbrhip.read_mip(maps.irradiance_map, 0)
    fresh_map = cube_texture(texels)
    maps2 = pbrhip.PBR_IBLMaps()
    maps2.irradiance_map, maps2.brdf_lut, maps2.tex_specular_env_map = fresh_map, maps.brdf_lut, maps.tex_specular_env_map
    lp2 = L.PBR_MakeLightingPass(C.byref(gb), C.byref(maps2), W, H)
    third = shade(lp2)
    assert second.tobytes() == third.tobytes()
    L.PBR_DestroyLightingPass(lp2); L.PBR_DestroyLightingPass(lp)
    L.GPU_DestroyTexture(fresh_map)
    L.PBR_DestroyGBuffer(C.byref(gb)); L.PBR_DestroyIBLMaps(C.byref(maps)); L.GPU_DestroyTexture(env_tex)


def test_kernel_abi_rejects_bad_arguments(gpu):
    """pbrk_sh9_* launch nothing for a bad extent, range or pointer"""
    L = gpu
    tex = cube_texture(cube_of(5))
    p = L.GPUX_TextureDevicePtr(tex, 0)
    try:
        assert L.pbrk_sh9_scratch_bytes(0) == 0 and L.pbrk_sh9_scratch_bytes(16385) == 0
        assert L.pbrk_sh9_scratch_bytes(1) == 216 and L.pbrk_sh9_scratch_bytes(16384) >= 216
        ok = (p, 5, 0, 6, 0, 5, p, p, None)
        for i, v in ((0, None), (1, 0), (1, 16385), (2, -1), (2, 6), (3, 7), (3, 0), (4, -1), (4, 5), (5, 6), (6, None), (7, None), (0, p + 4), (7, p + 4)):
            args = list(ok); args[i] = v
            assert L.pbrk_sh9_project(*args) != 0, (i, v)
        ok = (p, p, 5, 0, 6, 0, 5, None)
        for i, v in ((0, None), (1, None), (2, 0), (2, 16385), (3, 6), (4, 0), (5, 5), (6, 6), (1, p + 8), (0, p + 4)):
            args = list(ok); args[i] = v
            assert L.pbrk_sh9_irradiance(*args) != 0, (i, v)
        L.GPU_WaitUntilIdle()
        assert np.array_equal(__import__("pbrhip").read_mip(tex, 0), cube_of(5))          # nothing ran
    finally:
        L.GPU_DestroyTexture(tex)


class _Errors:
    def __init__(self, L):
        self.L, self.msgs = L, []
        self.cb = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)(lambda m, u: self.msgs.append(m.decode()))

    def __enter__(self):
        self.L.GPUX_SetErrorHandler(C.cast(self.cb, C.c_void_p), None)
        return self

    def __exit__(self, *a):
        self.L.GPUX_SetErrorHandler(None, None)


def test_errors(gpu):
    """one message and nothing recorded for each bad argument of the two ops"""
    import pbrhip
    L = gpu
    cube = cube_texture(cube_of(5))
    flat = pbrhip.make_texture(pbrhip.Format_RGBA32F, 8, 8, 0, np.zeros((8, 8, 4), np.float32))
    half = pbrhip.make_texture(pbrhip.Format_RGBA16F, 8, 8, pbrhip.TextureFlag_Cubemap, np.zeros((6, 8, 8, 4), np.float16))
    buf = L.GPU_MakeBuffer(432, pbrhip.BufferFlag_CPU, None)
    small = L.GPU_MakeBuffer(208, pbrhip.BufferFlag_CPU, None)
    C.memset(buf.contents.data, 0x5A, 432)
    before = pbrhip.read_mip(cube, 0)
    g = L.GPU_MakeGraph()
    with _Errors(L) as e:
        for args, needle in (((flat, 0, 0, 6, 0, 8, buf, 0), "square RGBA32F cubemap"), ((half, 0, 0, 6, 0, 8, buf, 0), "square RGBA32F cubemap"),
                             ((cube, 0, 0, 6, 0, 5, small, 0), "buffer too small"), ((cube, 0, 0, 6, 0, 5, buf, 224), "buffer too small"),
                             ((cube, 0, 0, 6, 0, 5, buf, 4), "multiple of 8"), ((cube, 0, 0, 6, 3, 3, buf, 0), "empty"),
                             ((cube, 0, 0, 6, 0, 6, buf, 0), "out-of-range"), ((cube, 0, 2, 2, 0, 5, buf, 0), "empty"),
                             ((cube, 0, 0, 7, 0, 5, buf, 0), "out-of-range"), ((cube, 1, 0, 6, 0, 5, buf, 0), "bad arguments")):
            e.msgs.clear()
            L.GPUX_OpProjectSH9(g, *args)
            assert len(e.msgs) == 1 and needle in e.msgs[0], (needle, e.msgs)
        for args, needle in (((buf, 0, flat, 0), "square RGBA32F cubemap"), ((buf, 0, half, 0), "square RGBA32F cubemap"),
                             ((small, 0, cube, 0), "buffer too small"), ((buf, 220, cube, 0), "multiple of 8"), ((buf, 224, cube, 0), "buffer too small"),
                             ((buf, 0, cube, 1), "bad arguments")):
            e.msgs.clear()
            L.GPUX_OpIrradianceFromSH9(g, *args)
            assert len(e.msgs) == 1 and needle in e.msgs[0], (needle, e.msgs)
        e.msgs.clear()
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)                              # nothing was recorded
        assert e.msgs == []
    assert C.string_at(buf.contents.data, 432) == b"\x5a" * 432
    assert np.array_equal(pbrhip.read_mip(cube, 0), before)
    L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(buf); L.GPU_DestroyBuffer(small)
    for t in (cube, flat, half):
        L.GPU_DestroyTexture(t)


def test_demo_writes_the_coefficients_of_its_environment(gpu, tmp_path):
    """pbr_demo ... sh9 FILE: the file holds the bits GPUX_OpProjectSH9 gives for level 0 of the loaded strip; every other line of
    the demo's output is what it prints without the argument"""
    import subprocess
    import pbrhip
    from pbrhip import synth
    L = gpu
    hdr = tmp_path / "cube_strip.hdr"
    hdr.write_bytes(synth.env_to_hdr_strip(synth.synth_env(64, seed=0x5EED0017), rle=True))
    exe = os.path.join(pbrhip.PKG_ROOT, "pbr_demo")
    sizes = ["32", "256", "64", "16", "320", "180"]                     # the sizes of the demo's end-to-end test
    path = tmp_path / "env.sh9"

    def lines(extra):
        out = subprocess.run([exe, str(hdr), *sizes, *extra], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return [l for l in out.stdout.splitlines() if not l.startswith("time_ms")]

    plain, with_sh = lines([]), lines(["sh9", str(path)])
    assert [l for l in with_sh if not l.startswith("sh9_sum")] == plain and plain[-1] == "ok 1"
    coef = np.zeros(27)
    assert L.PBR_ReadSH9File(str(path).encode(), coef.ctypes.data_as(C.POINTER(C.c_double))) == 0
    tex = L.PBR_MakeTextureFromHDRIFile(str(hdr).encode())
    try:
        assert coef.tobytes() == pbrhip.project_sh9(tex, 0).tobytes()
        want, S = R.project(pbrhip.read_mip(tex, 0))
        check_projection("demo file", coef.reshape(9, 3), want, S)
    finally:
        L.GPU_DestroyTexture(tex)
    printed = [float(l.split()[1]) for l in with_sh if l.startswith("sh9_sum")]
    assert len(printed) == 1 and abs(printed[0] - coef.sum()) <= 1e-12 * np.abs(coef).sum()
