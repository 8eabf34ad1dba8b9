"""K21 on the GPU: the GGX importance-sampled prefilter (GPUX_OpPrefilterGGX, csrc/k_prefilter_ggx.hip) against the numpy restatement of
tests/prefilter_ggx_ref.py, through the graph op, sub-ranges, hipGraph replay, the host layer and pbr_demo.

Criterion of every value comparison: the reference of a texel is the fp64 sum of (double) l.z (double) c over the K kept entries of the
library's own table, divided by (double) wsum, c being the restatement's fp32 trilinear colour.  The per-sample terms are bit-identical
by contract and non-negative (the cubes are), so any fp32 accumulation order errs by at most (K + 2) 2^-24 relative to first order:
asserted is |gpu - ref| <= (K + 2) 2^-23 ref.  The cubes are panorama_ref.hdr_cube: lognormal with one 5e4 texel, next to which a wrong
tap, a wrong level or a fused operation breaks the bound by orders of magnitude.

The kernel has one code path; what switches is the number of waves S that share a texel's samples (pggx_slices of
csrc/prefilter_ggx_core.h): 16 below 64^2, 4 from 64^2, 1 from 128^2 on; and, inside the loop, whether a sample blends two levels or
reads one (l1 == l0: a clamped lod, a source without mips)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panorama_ref as P  # noqa: E402
import prefilter_ggx_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-3.0)


@pytest.fixture(scope="module")
def env_of(gpu):
    """(n, with chain) -> (texture, the bordered numpy twins of its levels as the GPU holds them); made once, shared, never written"""
    import pbrhip
    made = {}

    def get(n, chain=True):
        if (n, chain) not in made:
            flags = pbrhip.TextureFlag_Cubemap | (pbrhip.TextureFlag_HasMipmaps if chain else 0)
            tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, n, n, flags, P.hdr_cube(n, 0x2100 + n))
            twins = R.bordered_levels([pbrhip.read_mip(tex, m) for m in range(tex.contents.mip_level_count)])
            for b in twins:
                b.setflags(write=False)
            made[(n, chain)] = (tex, twins)
        return made[(n, chain)]

    yield get
    for tex, _ in made.values():
        gpu.GPU_DestroyTexture(tex)


def target(size0, chain=True):
    """an RGBA32F cube whose every level holds the sentinel"""
    import pbrhip
    tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, size0, size0,
                              pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_StorageImage | (pbrhip.TextureFlag_HasMipmaps if chain else 0))
    for m in range(tex.contents.mip_level_count):
        n = max(1, size0 >> m)
        pbrhip.upload_mip(tex, m, np.full((6, n, n, 4), SENTINEL, np.float32))
    return tex


def run(L, g):
    L.GPU_GraphSubmit(g)
    L.GPU_GraphWait(g)


def table_of(env_tex, r, count, bias):
    import pbrhip
    return pbrhip.prefilter_ggx_samples(r, count, env_tex.contents.width, env_tex.contents.mip_level_count, bias)


def check(label, got, twins, size, table, wsum, faces=range(6)):
    """the criterion above on faces `faces` of a size^2 level; alpha is 1"""
    K = len(table)
    assert (got[..., 3] == 1).all(), label
    for f in faces:                                                           # face by face: bounds the temporaries of a big level
        want = R.prefilter_f64(twins, R.texel_dirs(size, [f])[0], table, wsum)
        g = got[f, ..., :3].astype(np.float64)
        if K == 0:                                                            # 0 / 0 on both sides
            assert np.isnan(g).all() and np.isnan(want).all(), label
            continue
        assert (want > 0).all()
        err = np.abs(g - want) / want
        worst = float(err.max())
        assert worst <= (K + 2) * 2.0 ** -23, (label, f, K, worst, np.unravel_index(int(err.argmax()), err.shape))


# (env size, env has its chain, size of the target cube, target mip): what each can break
SHAPES = [(32, True, 16, 0),     # 16^2: 1536 texels = 24 waves of 64, every one full
          (32, True, 16, 1),     # 8^2: 384 texels, 6 waves
          (32, True, 16, 3),     # 2^2: 24 texels in one wave, 40 idle lanes shadowing the last texel
          (32, True, 16, 4),     # 1^2: six lanes; every texel of +-Z takes the (1, 0, 0) up vector
          (24, True, 12, 0),     # source levels 24, 12, 6, 3, 1 and a 12^2 target: nothing is a power of two (the IEEE quotient by n)
          (24, True, 12, 1),     # 6^2
          (24, True, 12, 2),     # 3^2: the +-Z face centres take the other up vector, their neighbours do not
          (8, False, 8, 0)]      # a source of one level: every sample reads level 0 alone
COMBOS = [(r, n, b) for r in (0.05, 0.25, 0.5, 1.0) for n in (1, 16, 64) for b in (1.0, -4.0, 8.0)]
# bias -4 drives the samples into level 0 and fractional low lods, where the sun is one sharp texel; bias +8 makes all of them (from
# roughness 0.25 on) the 1^2 level, where every tap is apron or corner; N = 1 at roughness 1 keeps no sample at all: 0 / 0


@pytest.mark.parametrize("n_env,chain,size0,mip", SHAPES)
def test_level_is_within_the_accumulation_bound(gpu, env_of, n_env, chain, size0, mip):
    import pbrhip
    env, twins = env_of(n_env, chain)
    size = max(1, size0 >> mip)
    dst = target(size0)
    try:
        for r, count, bias in COMBOS + ([(r, 1024, 1.0) for r in (0.05, 0.25, 0.5, 1.0)] if size == 8 and not chain else []):
            pbrhip.prefilter_ggx(env, dst, mip, r, count, bias)
            table, wsum = table_of(env, r, count, bias)
            check(f"env {n_env} -> {size}^2 r {r} N {count} bias {bias}", pbrhip.read_mip(dst, mip), twins, size, table, wsum)
        for m in range(dst.contents.mip_level_count):                          # the other levels were not touched
            if m != mip:
                assert (pbrhip.read_mip(dst, m) == SENTINEL).all(), m
    finally:
        gpu.GPU_DestroyTexture(dst)


@pytest.mark.parametrize("size", [63, 64, 127, 128])
def test_both_sides_of_every_slice_count_switch(gpu, env_of, size):
    """pggx_slices: 63 -> 16 waves per texel, 64 and 127 -> 4, 128 -> 1 (four waves of different texels).  N = 16 at roughness 0.5
    keeps 15 samples: with 16 slices one wave has none, with 4 the last has three; 63 and 127 leave a ragged last workgroup"""
    import pbrhip
    env, twins = env_of(32)
    dst = target(size, chain=False)
    try:
        pbrhip.prefilter_ggx(env, dst, 0, 0.5, 16, 1.0)
        table, wsum = table_of(env, 0.5, 16, 1.0)
        assert len(table) == 15
        check(f"{size}^2", pbrhip.read_mip(dst, 0), twins, size, table, wsum)
    finally:
        gpu.GPU_DestroyTexture(dst)


def test_many_workgroups(gpu, env_of):
    """env 128^2 with its chain -> 64^2 at N = 256: 384 workgroups of four slices, lods from 3.3 to 6.4 across four source levels"""
    import pbrhip
    env, twins = env_of(128)
    dst = target(64, chain=False)
    try:
        pbrhip.prefilter_ggx(env, dst, 0, 0.5, 256, 1.0)
        table, wsum = table_of(env, 0.5, 256, 1.0)
        assert len(np.unique(np.floor(table[:, 3]))) >= 3
        check("128 -> 64^2", pbrhip.read_mip(dst, 0), twins, 64, table, wsum)
    finally:
        gpu.GPU_DestroyTexture(dst)


def test_constant_cube_gives_the_constant(gpu):
    import pbrhip
    v = np.array([0.37, 11.0, 5.0e4, 1.0], np.float32)
    env = pbrhip.make_texture(pbrhip.Format_RGBA32F, 8, 8, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps,
                              np.ascontiguousarray(np.broadcast_to(v, (6, 8, 8, 4))))
    dst = target(3, chain=False)
    try:
        for r, count, bias in [(0.05, 16, 1.0), (0.5, 1024, 1.0), (1.0, 64, -4.0)]:
            pbrhip.prefilter_ggx(env, dst, 0, r, count, bias)
            K = len(table_of(env, r, count, bias)[0])
            got = pbrhip.read_mip(dst, 0)
            assert (np.abs(got[..., :3].astype(np.float64) / v[:3] - 1) <= (K + 2) * 2.0 ** -23).all() and (got[..., 3] == 1).all()
    finally:
        gpu.GPU_DestroyTexture(dst); gpu.GPU_DestroyTexture(env)


# ---- sub-ranges, determinism ----
def level_bytes(tex, mip):
    import pbrhip
    return pbrhip.read_mip(tex, mip).copy()


@pytest.mark.parametrize("size0,mip", [(16, 0), (64, 0)])                      # 16 slices; 4 slices
def test_sub_ranges_write_the_same_bytes_and_nothing_else(gpu, env_of, size0, mip):
    import pbrhip
    env, _ = env_of(32)
    whole, part, halves = target(size0), target(size0), target(size0)
    n = size0 >> mip
    try:
        args = (mip, 0.25, 64, 1.0)
        pbrhip.prefilter_ggx(env, whole, *args)
        want = level_bytes(whole, mip)
        assert (want != SENTINEL).all()
        pbrhip.prefilter_ggx(env, part, *args, faces=(2, 5), rows=(3, 11))
        got = level_bytes(part, mip)
        inside = np.zeros((6, n, n), bool)
        inside[2:5, 3:11, :] = True
        assert (got[~inside] == SENTINEL).all()
        assert got[inside].tobytes() == want[inside].tobytes()
        pbrhip.prefilter_ggx(env, halves, *args, faces=(0, 6), rows=(0, 5))
        pbrhip.prefilter_ggx(env, halves, *args, faces=(0, 6), rows=(5, n))
        assert level_bytes(halves, mip).tobytes() == want.tobytes()
        pbrhip.prefilter_ggx(env, halves, *args, faces=(0, 2), rows=(0, n))
        pbrhip.prefilter_ggx(env, halves, *args, faces=(2, 6), rows=(0, n))
        assert level_bytes(halves, mip).tobytes() == want.tobytes()
    finally:
        for t in (whole, part, halves):
            gpu.GPU_DestroyTexture(t)


@pytest.mark.parametrize("size", [8, 64, 128])                                 # 16, 4 and 1 slices
def test_the_same_op_twice_gives_the_same_bytes(gpu, env_of, size):
    import pbrhip
    env, _ = env_of(32)
    a, b = target(size, chain=False), target(size, chain=False)
    try:
        pbrhip.prefilter_ggx(env, a, 0, 0.5, 64, 1.0)
        pbrhip.prefilter_ggx(env, b, 0, 0.5, 64, 1.0)
        first = level_bytes(a, 0)
        pbrhip.prefilter_ggx(env, a, 0, 0.5, 64, 1.0)
        assert first.tobytes() == level_bytes(b, 0).tobytes() == level_bytes(a, 0).tobytes()
    finally:
        gpu.GPU_DestroyTexture(a); gpu.GPU_DestroyTexture(b)


# ---- ordering ----
def test_effects_are_followed(gpu):
    """the apron is rebuilt after a write to the environment (GPU_GraphWait resets a graph, so the op is recorded again for the second
    submission) and is a timed entry of its own; a panorama of the target behind the op in the same graph sees the new level"""
    import pbrhip
    L = gpu
    old, new = P.hdr_cube(8, 0x2101), P.hdr_cube(8, 0x2102)
    env = pbrhip.make_texture(pbrhip.Format_RGBA32F, 8, 8, pbrhip.TextureFlag_Cubemap, old)
    dst = target(4, chain=False)
    pano = pbrhip.make_texture(pbrhip.Format_RGBA32F, 16, 8, 0)
    table, wsum = table_of(env, 0.5, 16, 1.0)
    nrm = R.texel_dirs(4)
    g = L.GPU_MakeGraph()
    L.GPUX_EnableOpTiming(1)
    try:
        names = []
        for k, data in enumerate((old, new, new)):
            L.GPUX_OpPrefilterGGX(g, env, dst, 0, 0.5, 16, 1.0, 0, 6, 0, 4)
            L.GPUX_OpCubeToPanorama(g, dst, 0, pano, 0)
            run(L, g)
            names.append([L.GPUX_GraphTimedOpName(g, i).decode() for i in range(L.GPUX_GraphTimedOpCount(g))])
            got = pbrhip.read_mip(dst, 0)
            check(f"submission {k}", got, R.bordered_levels([data]), 4, table, wsum)
            assert pbrhip.read_mip(pano, 0).tobytes() == P.panorama(got, 16, 8).tobytes(), k
            if k == 0:
                pbrhip.upload_mip(env, 0, new)
        tail = ["K21.prefilter_ggx.mip0", "apron.panorama", "K20.cube_to_panorama"]
        assert names == [["apron.prefilter_ggx"] + tail] * 2 + [tail], names
    finally:
        L.GPUX_EnableOpTiming(0)
        L.GPU_DestroyGraph(g)
        for t in (env, dst, pano):
            L.GPU_DestroyTexture(t)


def test_graph_replay_leaves_the_op_on_the_plain_path(gpu, env_of):
    import pbrhip
    L = gpu
    env, _ = env_of(32)
    plain, dst = target(8, chain=False), target(8, chain=False)
    g = L.GPU_MakeGraph()
    try:
        pbrhip.prefilter_ggx(env, plain, 0, 0.25, 64, 1.0)
        want = level_bytes(plain, 0)
        L.GPUX_SetGraphReplay(1)
        for _ in range(2):
            pbrhip.upload_mip(dst, 0, np.full((6, 8, 8, 4), SENTINEL, np.float32))
            L.GPUX_OpPrefilterGGX(g, env, dst, 0, 0.25, 64, 1.0, 0, 6, 0, 8)
            run(L, g)
            assert level_bytes(dst, 0).tobytes() == want.tobytes()
        s = [C.c_uint64(0) for _ in range(3)]
        L.GPUX_GraphReplayStats(g, *[C.byref(v) for v in s])
        assert [v.value for v in s] == [0, 0, 0]
    finally:
        L.GPUX_SetGraphReplay(-1)
        L.GPU_DestroyGraph(g); L.GPU_DestroyTexture(dst); L.GPU_DestroyTexture(plain)


# ---- argument checks ----
def test_bad_arguments_are_one_error_each_and_record_nothing(gpu, env_of):
    import pbrhip
    L = gpu
    messages = []
    handler = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)(lambda msg, user: messages.append(msg.decode()))
    env, _ = env_of(32)
    dst = target(8)
    half_cube = pbrhip.make_texture(pbrhip.Format_RGBA16F, 4, 4, pbrhip.TextureFlag_Cubemap)
    flat = pbrhip.make_texture(pbrhip.Format_RGBA32F, 4, 4, 0)
    sun = L.PBR_MakeSunDepthPass(64)
    g = L.GPU_MakeGraph()
    L.GPUX_SetErrorHandler(C.cast(handler, C.c_void_p), None)
    L.GPUX_EnableOpTiming(1)
    ok = (0, 0.5, 16, 1.0, 0, 6, 0, 8)
    nan, inf = float("nan"), float("inf")
    try:
        bad = [(None, dst) + ok, (env, None) + ok,                                               # NULL
               (half_cube, dst) + ok, (flat, dst) + ok, (env, half_cube) + ok, (env, flat) + ok,   # formats, not a cube
               (dst, dst) + ok,                                                                  # the source as its own target
               (env, dst, 4) + ok[1:],                                                           # a mip past the chain
               (env, dst, 0, 0.0) + ok[2:], (env, dst, 0, -0.5) + ok[2:], (env, dst, 0, 1.0001) + ok[2:], (env, dst, 0, nan) + ok[2:],
               (env, dst, 0, 0.5, 0) + ok[3:], (env, dst, 0, 0.5, 4097) + ok[3:],                # the count
               (env, dst, 0, 0.5, 16, inf) + ok[4:], (env, dst, 0, 0.5, 16, nan) + ok[4:],       # the bias
               (env, dst, 0, 0.5, 16, 1.0, 3, 3, 0, 8), (env, dst, 0, 0.5, 16, 1.0, 0, 7, 0, 8),   # faces: empty, past 6
               (env, dst, 0, 0.5, 16, 1.0, 0, 6, 5, 5), (env, dst, 0, 0.5, 16, 1.0, 0, 6, 0, 9),   # rows: empty, past the level
               (env, dst, 1, 0.5, 16, 1.0, 0, 6, 0, 5)]                                           # rows of level 0 on the 4^2 level
        for k, args in enumerate(bad):
            L.GPUX_OpPrefilterGGX(g, *args)
            assert len(messages) == k + 1, (k, args[2:], messages)
        L.GPU_OpPrepareRenderPass(g, L.PBR_SunDepthRenderPass(sun))
        L.GPU_OpBeginRenderPass(g)
        L.GPUX_OpPrefilterGGX(g, env, dst, *ok)                               # inside a render pass
        L.GPU_OpEndRenderPass(g)
        assert len(messages) == len(bad) + 1 and "inside a render pass" in messages[-1], messages
        run(L, g)
        assert L.GPUX_GraphTimedOpCount(g) == 0                              # nothing was recorded
        for m in range(dst.contents.mip_level_count):
            assert (pbrhip.read_mip(dst, m) == SENTINEL).all()
        assert all(m.startswith("GPUX_OpPrefilterGGX: ") for m in messages), messages
    finally:
        L.GPUX_EnableOpTiming(0)
        L.GPUX_SetErrorHandler(None, None)
        L.GPU_DestroyGraph(g)
        L.PBR_DestroySunDepthPass(sun)
        for t in (dst, half_cube, flat):
            L.GPU_DestroyTexture(t)


# ---- host layer ----
def test_host_layer_bakes_level_zero_as_before_and_the_rest_by_the_op(gpu, env_of):
    import pbrhip
    L = gpu
    env, _ = env_of(32)
    spec, old, one = target(16), target(16), target(16)
    try:
        L.PBR_GenPrefilteredEnvMapGGX(env, spec, 2, 64)
        L.PBR_GenPrefilteredEnvMap(env, old, 2)
        assert level_bytes(spec, 0).tobytes() == level_bytes(old, 0).tobytes()
        for i in (1, 2, 3):
            pbrhip.prefilter_ggx(env, one, i, min(1.0, i / 4), 64, 1.0)
            assert level_bytes(spec, i).tobytes() == level_bytes(one, i).tobytes(), i
            assert level_bytes(spec, i).tobytes() != level_bytes(old, i).tobytes(), i
        assert (pbrhip.read_mip(spec, 4) == SENTINEL).all()                   # 1^2 is below min_size
    finally:
        for t in (spec, old, one):
            L.GPU_DestroyTexture(t)


def test_demo_bakes_the_specular_map_with_the_keyword(gpu, tmp_path):
    """pbr_demo ... ggx 64: the same line names, the same specular_mip0_sum, another specular_mip1_sum"""
    import pbrhip
    from pbrhip import synth
    hdr = tmp_path / "cube_strip.hdr"
    hdr.write_bytes(synth.env_to_hdr_strip(synth.synth_env(64, seed=0x5EED0021), rle=True))
    exe = os.path.join(pbrhip.PKG_ROOT, "pbr_demo")
    base = [exe, str(hdr), "16", "64", "32", "8", "64", "36"]
    runs = []
    for extra in ([], ["ggx", "64"]):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l.split() for l in out.stdout.splitlines()]
        assert lines[-1] == ["ok", "1"]
        runs.append(lines)
    plain, ggx = runs
    assert [l[0] for l in plain] == [l[0] for l in ggx]
    value = lambda lines, key: [l[1] for l in lines if l[0] == key]  # noqa: E731
    assert value(plain, "specular_mip0_sum") == value(ggx, "specular_mip0_sum") and len(value(ggx, "specular_mip0_sum")) == 1
    assert value(plain, "specular_mip1_sum") != value(ggx, "specular_mip1_sum")
    assert subprocess.run(base + ["ggx", "0"], capture_output=True, text=True, timeout=120).returncode == 2
