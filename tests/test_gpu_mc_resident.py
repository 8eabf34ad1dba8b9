"""Levels of at most 16^2 texels kept resident in LDS (k_mc_region.hip, header 2k: k_mc_resident -- per tile the proved samples run
test-free face by face, every other sample once with each lane on its own face) against the direct kernel, against the kernel the
level ran before (pbrk_mc_set_resident(0)) and against itself under sharding.

256^2 outputs, the smallest with whole 16 x 16 tiles on every face: a tile spans one source texel at n_src = 16, its frames spread four
times as far as on C4 mip 4, so the proved share is at its lowest and the general pass does the most work.  n_src = 12 is no power of
two (the unfolded body) and fills its 18^2 blocks partly; 8 fills a quarter of them.  128^2 outputs take 8 x 8 tiles x 16 slices.  Tables: the whole table of the roughness, 1000
samples (the last mask word ragged) and 100 (at most one word per slice).

Two places where the test reads the request that set it more narrowly than written, and why:
  * "the off state took the region kernel" is asserted for 16 -> 256^2 alone.  The region kernel has never taken a level below 16^2 or
    an output below 256^2 (launch_mc_region), so with the switch off the other shapes run the level-in-LDS kernel, as they did before;
    there the test asserts that the region kernel did NOT run.  The 2e-5 comparison with the off state holds for all three.
  * the proved count is read from the kernel's own getter (pbrk_mc_resident_stats), not from the window counter: that one is pinned to
    0 on the 16^2 level by test_gpu_mc_certain_g1.py, whatever kernel serves it."""
import ctypes as C

import numpy as np
import pytest

from mc_cases import OUT, WINDOWS, level
from pbrhip import mc

pytestmark = pytest.mark.gpu

# (n_src, roughness, output size): 16 x 16 tiles x 4 slices at 256^2; 8 x 8 tiles x 16 slices at 128^2 (a table of 100 samples has
# fewer mask words than slices there)
SHAPES = [(16, 0.6, 256), (12, 0.6, 256), (8, 0.68, 256), (8, 0.68, 128), (16, 0.6, 128)]
TABLES = [None, 1000, 100]
REL, FLOOR = 2e-5, 1e-3                     # test_c4_every_texel_region_kernel_against_direct_kernel's bound for this comparison
assert OUT == 256


def _tile(out):
    return 16 if out >= 256 else 8


def _tiles(out):
    return 6 * (out // _tile(out)) ** 2


def _full(out):
    return [(0, 6, 0, out)]


def _resident_stats(L):
    buf = (C.c_uint64 * 4)()
    assert L.pbrk_mc_resident_stats(buf) == 0
    return dict(zip(("violations", "proved", "run_pairs", "general_pairs"), (int(v) for v in buf)))


def _run(L, bord, rough, n_tab, out, windows=None, resident=1, kernels=None):
    """One dispatch set (default: the whole level) into a cleared cube: ([6, out, out, 4] float32, counters)."""
    windows = windows or _full(out)
    mc.reset_counters(L)
    L.pbrk_mc_set_resident(resident)
    try:
        if kernels is None:
            data = mc.filter_windows(L, bord, rough, windows, out, n_tab)
        else:
            with mc.switches(L, kernels=kernels):
                data = mc.filter_windows(L, bord, rough, windows, out, n_tab)
    finally:
        L.pbrk_mc_set_resident(-1)                                       # the library's default
    c = mc.counters(L, "flag", "window", missing_ok=True)
    c.update(_resident_stats(L))
    c.update(mc.counters(L, "region", reset=True))
    return np.frombuffer(data, np.float32).reshape(6, out, out, 4), c


def _rel(a, b):
    return float((np.abs(a[..., :3].astype(np.float64) - b[..., :3]) / np.maximum(np.abs(b[..., :3]), FLOOR)).max())


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"n{s[0]}o{s[2]}")
def shape(request, gpu):
    n_src, rough, out = request.param
    # the counters exist after the first launch of a region-family kernel
    warm = mc.BorderedLevel(gpu, level(16))
    mc.filter_windows(gpu, warm, 0.6, [(0, 1, 0, 16)], OUT, 32)
    warm.free()
    bord = mc.BorderedLevel(gpu, level(n_src))
    ones = mc.BorderedLevel(gpu, np.ones((6, n_src, n_src, 4), np.float32))
    yield n_src, rough, out, bord, ones
    bord.free()
    ones.free()


@pytest.mark.parametrize("n_tab", TABLES, ids=lambda n: f"tab{n or 'full'}")
def test_against_direct_kernel_and_off_state(gpu, shape, n_tab):
    L = gpu
    n_src, rough, out, bord, _ = shape
    tiles, texels = _tiles(out), _tile(out) ** 2
    n = n_tab or mc.prefilter_table(L, rough)[1]
    assert n >= 1000 or n_tab is not None, n
    got, c = _run(L, bord, rough, n_tab, out)
    direct, cd = _run(L, bord, rough, n_tab, out, kernels=(0, 0))
    off, co = _run(L, bord, rough, n_tab, out, resident=0)
    # which kernel ran: the resident one counts pairs, the direct one enters no counter, the off state is the parent's choice
    assert c["run_pairs"] + c["general_pairs"] > 0 and c["slices"] == 16 * tiles and c["healed"] == 0, c
    assert cd["slices"] == 0 and cd["run_pairs"] + cd["general_pairs"] == 0, cd
    assert co["run_pairs"] + co["general_pairs"] == 0, co
    if n_src == 16 and out >= 256:
        assert co["slices"] > 0 and co["flags"] > co["flag_samples"] and co["healed"] == 0, co
    else:
        assert co["slices"] == 0, co
    e_direct, e_off = _rel(got, direct), _rel(got, off)
    print(f"n_src {n_src} -> {out}^2 n_tab {n}: vs direct {e_direct:.3e} / {REL:.0e}, vs off state {e_off:.3e} / {REL:.0e}; proved {c['proved']} of "
          f"{c['flag_samples']} ({c['proved'] / c['flag_samples']:.3f}), flags per sample {c['flags'] / c['flag_samples']:.3f}")
    assert np.array_equal(got[..., 3].view(np.uint32), direct[..., 3].view(np.uint32))
    assert e_direct < REL, (e_direct, REL)
    assert e_off < REL, (e_off, REL)
    # counters: no proof failed in any lane, the proved path is taken, and every (texel, sample) pair is taken exactly once
    assert c["violations"] == 0, c
    assert c["flag_samples"] == n * tiles and c["flags"] >= c["flag_samples"], c
    assert 0 < c["proved"] < c["flag_samples"], c
    assert c["run_pairs"] == texels * c["proved"], c
    assert c["run_pairs"] + c["general_pairs"] == n * texels * tiles, c


@pytest.mark.parametrize("n_tab", TABLES, ids=lambda n: f"tab{n or 'full'}")
def test_level_of_ones_against_direct_kernel(gpu, shape, n_tab):
    """A level of ones: a pair taken twice or missed changes a sum by a whole weight (1e-4 of it and more).  RGB within 2e-6 of the
    direct kernel's, alpha bit-equal.

    Measured on MI355X, worst |difference| over all texels against the direct kernel, whole table / 1000 / 100 samples:
        256^2: n_src 16 6.6e-7 / 4.5e-8 / 1.1e-8, n_src 12 6.6e-7 / 4.5e-8 / 1.1e-8, n_src 8 4.8e-7 / 4.5e-8 / 9.3e-9
        128^2: n_src 8 1.2e-7 / 3.0e-8 / 7.5e-9, n_src 16 1.8e-7 / 4.5e-8 / 9.3e-9
    The bound is what the kernel's word sums are for (k_mc_region.hip, "Word sums"): on ones the direct kernel's lerps return exactly 1
    and a weight enters its sum with one rounding, while tap_accumulate adds a sample's four tap weights with four.  Added straight
    into a slice's sum of up to 0.56 (half an ulp: 3e-8), the 8192 roundings of a 2048-sample slice walk 1.5e-6, four slices 3e-6, over
    pi 1e-6 rms, and the worst of 1.2 million sums lay at 2.0 - 2.7e-6 -- where the region kernel this one replaces on 16 -> 256^2
    stands too (2.62e-6)."""
    L = gpu
    n_src, rough, out, _, ones = shape
    flat, cf = _run(L, ones, rough, n_tab, out)
    flat_direct, _ = _run(L, ones, rough, n_tab, out, kernels=(0, 0))
    assert cf["violations"] == 0 and cf["run_pairs"] > 0, cf
    worst = float(np.abs(flat[..., :3].astype(np.float64) - flat_direct[..., :3]).max())
    print(f"ones, n_src {n_src} -> {out}^2 n_tab {n_tab or 'full'}: worst |difference| {worst:.3e} / 2e-6")
    assert np.array_equal(flat[..., 3].view(np.uint32), flat_direct[..., 3].view(np.uint32))
    assert worst <= 2e-6, worst


@pytest.mark.parametrize("n_tab", [None, 1000], ids=lambda n: f"tab{n or 'full'}")
def test_row_windows_and_single_faces_equal_the_full_dispatch(gpu, shape, n_tab):
    """Windows that start and end inside a tile (53 + 37 rows), at the pole rows of faces +-X, one row, the last rows, and every face
    alone: bit for bit."""
    L = gpu
    n_src, rough, out, bord, _ = shape
    full, _ = _run(L, bord, rough, n_tab, out)
    windows = WINDOWS if out == OUT else [(0, 2, 24, 16), (0, 2, 88, 16), (2, 6, 53, 37)]
    for f0, f1, y0, rows in windows + [(0, 6, 5, 1), (1, 3, out - 5, 5)] + [(f, f + 1, 0, out) for f in range(6)]:
        win, c = _run(L, bord, rough, n_tab, out, [(f0, f1, y0, rows)])
        assert c["violations"] == 0 and c["run_pairs"] > 0, c
        assert win[f0:f1, y0:y0 + rows].tobytes() == full[f0:f1, y0:y0 + rows].tobytes(), (f0, f1, y0, rows)
        rest = win.copy()
        rest[f0:f1, y0:y0 + rows] = 0.0
        assert not rest.any(), (f0, f1, y0, rows)                       # nothing outside the window is written


def test_unit_path_equals_the_full_dispatch(gpu):
    """256^2 from a 16^2 level through PBR_RecordUnits, three ragged row shards per face, against one unit for the whole level."""
    import pbrhip
    from pbrhip import synth
    L = gpu
    S, mip = 512, 1
    tex = mc.env_texture(synth.synth_env(256, seed=0x5EED00AD))
    try:
        with mc.dispatch_prefilter_units(L, tex, S, [pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, mip, 0, 6, 0, S >> mip, 0.0)]) as maps:
            c = _resident_stats(L)
            full = pbrhip.read_mip(maps.tex_specular_env_map, mip).copy()
        assert c["violations"] == 0 and c["run_pairs"] > 0 and _n_tab(c) > 0, c
        units = []
        for f in range(6):
            cuts = (0, 5 + f, 131 - 2 * f, S >> mip)
            units += [pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, mip, f, f + 1, cuts[k], cuts[k + 1], 0.0) for k in range(3)]
        with mc.dispatch_prefilter_units(L, tex, S, units) as maps:
            c = _resident_stats(L)
            got = pbrhip.read_mip(maps.tex_specular_env_map, mip)
            assert c["violations"] == 0 and c["run_pairs"] > 0, c
            assert np.array_equal(got.view(np.uint32), full.view(np.uint32))
            assert float(np.abs(got[..., :3]).max()) > 0.0
    finally:
        L.GPU_DestroyTexture(tex)


def _n_tab(c):
    """Samples per texel of a full 256^2 dispatch, from its pair counters (a whole number: every texel takes every sample once)."""
    pairs = c["run_pairs"] + c["general_pairs"]
    assert pairs % (256 * _tiles(OUT)) == 0, c
    return pairs // (256 * _tiles(OUT))


# ---- region_bin's proof replayed on the host ----
_FACE = [lambda x, y, z: (-z, -y, x), lambda x, y, z: (z, -y, -x), lambda x, y, z: (x, z, y),
         lambda x, y, z: (x, -z, -y), lambda x, y, z: (x, -y, z), lambda x, y, z: (-x, -y, -z)]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _frames(face, ix, iy, size):
    """face_texel_dir, tangent_of and the bitangent (pbr_device.h) in float64: R, T, B of shape ix.shape + (3,)."""
    sc = 2.0 * ((ix + 0.5) / size - 0.5)
    tc = 2.0 * ((iy + 0.5) / size - 0.5)
    one = np.ones_like(sc)
    r = [(one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one)][face]
    R = _unit(np.stack(r, -1))
    some = np.array([np.float32(12.123825810901), np.float32(6.11831989512), np.float32(-5.12039214121)], np.float64)
    T = _unit(np.cross(R, some))
    return R, T, np.cross(T, R)


def _proved_bounds(tab, n_src, size):
    """(lo, hi): the (tile, sample) pairs region_bin proves when every inequality must hold with a margin EPS to spare / may miss
    by EPS.  The kernel evaluates the same expressions in fp32 with v_rcp_f32 / v_sqrt_f32: about ten roundings of 2^-24 and two of
    one ulp on quantities of order one (EPS = 1e-5) or of at most n_src + 2 texels (EPS_T = 1e-4), so its count lies between the two."""
    EPS, EPS_T = 1e-5, 1e-4
    nf, half_n, off = float(n_src), 0.5 * n_src, 0.5 * n_src + 0.5
    e = tab.astype(np.float64)
    lo = hi = 0
    ty, tx = np.meshgrid(np.arange(size // 16), np.arange(size // 16), indexing="ij")
    ly, lx = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    for face in range(6):
        R, T, B = _frames(face, (tx[..., None, None] * 16 + lx).astype(np.float64), (ty[..., None, None] * 16 + ly).astype(np.float64), size)
        Rc, Tc, Bc = _frames(face, tx * 16 + 8.0, ty * 16 + 8.0, size)
        d2 = sum(((a - b[:, :, None, None, :]) ** 2).sum(-1) for a, b in ((R, Rc), (T, Tc), (B, Bc)))
        delta = (np.sqrt(d2).max((-1, -2)) * np.float32(0.70710678) * np.float32(1.001) + np.float32(4e-6))[..., None]      # [ty, tx, 1]
        L = e[:, 0, None] * Bc[:, :, None, :] + e[:, 1, None] * Tc[:, :, None, :] + e[:, 2, None] * Rc[:, :, None, :]   # [ty, tx, sample, 3]
        dd = np.float32(1.41421357) * delta
        sure = np.zeros(L.shape[:3], bool); maybe = np.zeros_like(sure)
        flag_sure = np.zeros(L.shape[:3], int); flag_maybe = np.zeros_like(flag_sure)
        for f in range(6):
            sc, tc, ma = _FACE[f](L[..., 0], L[..., 1], L[..., 2])
            mlo = ma - delta
            with np.errstate(divide="ignore", invalid="ignore"):
                rl = 1.0 / mlo
                gu, gv = (np.abs(sc) + delta) * rl, (np.abs(tc) + delta) * rl
                mu = delta * np.sqrt(gu * gu + 1.0) * rl * half_n * np.float32(1.0001) + np.float32(0.05)
                mv = delta * np.sqrt(gv * gv + 1.0) * rl * half_n * np.float32(1.0001) + np.float32(0.05)
                uc, vc = sc / ma * half_n + off, tc / ma * half_n + off
            for sg, flags, proof in ((1.0, flag_sure, sure), (-1.0, flag_maybe, maybe)):
                # sg = 1: "flagged" generously and "proved" strictly (a lower bound of the proved count); sg = -1: the other way round
                onf = (ma + dd - np.abs(sc) >= -sg * EPS) & (ma + dd - np.abs(tc) >= -sg * EPS)
                near = mlo > 0.2 + sg * EPS                                 # a comparison with NaN (ma = 0) is False: flagged, not proved
                miss = near & ((uc + mu < -sg * EPS_T) | (uc - mu >= nf + 1.0 + sg * EPS_T) | (vc + mv < -sg * EPS_T) | (vc - mv >= nf + 1.0 + sg * EPS_T))
                flags += onf & ~miss
                proof |= (near & (ma - dd - np.abs(sc) > sg * EPS) & (ma - dd - np.abs(tc) > sg * EPS)
                          & (uc - mu >= sg * EPS_T) & (uc + mu < nf + 1.0 - sg * EPS_T) & (vc - mv >= sg * EPS_T) & (vc + mv < nf + 1.0 - sg * EPS_T))
        lo += int((sure & (flag_sure == 1)).sum())
        hi += int((maybe & (flag_maybe <= 1)).sum())
    return lo, hi


def test_proved_count_equals_a_host_replay_of_the_proof(gpu):
    """n_src 16, 100 samples, every 16 x 16 tile of a 256^2 cube: the kernel's proved count lies between the replay's two counts."""
    L = gpu
    rough, n_tab = 0.6, 100
    tab = np.zeros((8192, 4), dtype=np.float32)
    alpha = C.c_float()
    assert L.pbrk_host_prefilter_table(8192, rough, tab.ctypes.data_as(C.c_void_p), C.byref(alpha)) >= n_tab
    lo, hi = _proved_bounds(tab[:n_tab], 16, OUT)
    bord = mc.BorderedLevel(L, level(16))
    try:
        _, c = _run(L, bord, rough, n_tab, OUT)
    finally:
        bord.free()
    print(f"proved on the device {c['proved']}, replay {lo} .. {hi}: {hi - lo} pairs within the rounding margin, of {n_tab * _tiles(OUT)}")
    assert c["violations"] == 0 and lo > 0
    assert lo <= c["proved"] <= hi, (lo, c["proved"], hi)
    # the margin is a band of relative width ~1e-5 around inequalities whose two sides vary by order one over the pairs
    assert hi - lo <= max(8, n_tab * _tiles(OUT) // 1000), (lo, hi)
