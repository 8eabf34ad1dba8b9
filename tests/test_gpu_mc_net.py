"""The region kernel without its completeness net (k_mc_region.hip, header 2l; pbrk_mc_set_net) against the instantiation that keeps it.
The net -- the pair count of every wave, the credits of proved and cut samples, the count-only walk of an absorbed word's unproved
samples, the check against expect[] and heal_slice -- adds nothing to any sum, so net=0 must give the bytes of net=1 on every shape
that has a net-less instantiation: quarter faces with both tiles, whole faces, the 34^2 shape, each folded and unfolded.
pbrk_mc_last_net() tells which instantiation a launch took.  The suite runs with the device counters on, where the default rule (-1)
keeps the net: the two states are asked for by name here.  The net-less kernel also ends a pass at the first absorbed word behind which
the slice's word maxima never rise again; under the counters it credits the words it leaves, so the absorbed counts must agree as well.

256^2 outputs, the smallest the region kernel accepts.  Tables: roughness 0.03 (1389 samples: the launch cut and absorbed words) and
0.15 (8192 samples); each whole, its first 1000 samples (the last mask word ragged) and its first 100 (one phase)."""
import ctypes as C

import numpy as np
import pytest

import pbrhip
from mc_cases import FULL, OUT, WINDOWS, level
from pbrhip import mc

pytestmark = pytest.mark.gpu

# (n_src, tile32): quarter faces with the 16 x 16 x 4 and the 32 x 32 x 1 tile; the 66^2 whole face; the 34^2 shape; two levels whose
# edge is no power of two (quarter faces and a partly filled 66^2 whole face): the unfolded instantiations
SHAPES = [(128, 0), (128, 1), (64, 0), (32, 0), (96, 0), (48, 0)]
ROUGHS = [0.03, 0.15]
TABLES = [None, 1000, 100]
# three shards per face, cuts that are no multiple of 16 or 32 and differ per face; then every face on its own
SHARDS = [(f, f + 1, a, b - a) for f in range(6) for a, b in ((0, 5 + f), (5 + f, 131 - 2 * f), (131 - 2 * f, OUT))]
SINGLE_FACES = [(f, f + 1, 0, OUT) for f in range(6)]
C4_S, C4_MIN = 4096, 128


def _run(L, bord, rough, n_tab, tile32, net, windows=FULL):
    """One dispatch set into a cleared cube: (bytes, counters, pbrk_mc_last_net())."""
    with mc.switches(L, tile32=tile32, net=net):
        mc.reset_counters(L)
        data = mc.filter_windows(L, bord, rough, windows, OUT, n_tab)
        took = L.pbrk_mc_last_net()
        # missing_ok: the counters exist only once the region kernel has run in this process
        return data, mc.counters(L, "skip", "flag", "window", "region", reset=True, missing_ok=True), took


def _check_pair(on, off, tag):
    """on = a run with net=1, off = the same with net=0."""
    (d1, c1, t1), (d0, c0, t0) = on, off
    print(f"{tag}: net 1 -> healed {c1['healed']} of {c1['slices']}, absorbed {c1['abs_words']} words / {c1['abs_samples']} samples, "
          f"count-only {c1['count_only']}, proved {c1['proved']}; net 0 -> last_net {t0}, healed {c0['healed']} of {c0['slices']}, "
          f"absorbed {c0['abs_words']} / {c0['abs_samples']}, count-only {c0['count_only']}")
    assert t1 == 1 and t0 == 0, (tag, t1, t0)
    assert c1["healed"] == 0 and c1["slices"] > 0, (tag, c1)
    assert c0["healed"] == 0 and c0["count_only"] == 0, (tag, c0)
    assert c0["slices"] == c1["slices"], (tag, c0, c1)
    assert (c0["abs_words"], c0["abs_samples"]) == (c1["abs_words"], c1["abs_samples"]), (tag, c0, c1)
    assert (c0["flags"], c0["flag_samples"], c0["visits"], c0["proved"]) == (c1["flags"], c1["flag_samples"], c1["visits"], c1["proved"]), (tag, c0, c1)
    assert d0 == d1, f"{tag}: the bytes moved with the net off"


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"n{s[0]}t{s[1]}")
def shape(request, gpu):
    n_src, tile32 = request.param
    bord = mc.BorderedLevel(gpu, level(n_src))
    yield n_src, tile32, bord
    bord.free()


@pytest.mark.parametrize("n_tab", TABLES, ids=lambda n: f"tab{n or 'full'}")
@pytest.mark.parametrize("rough", ROUGHS, ids=lambda r: f"r{r}")
def test_net_off_keeps_the_bytes(gpu, shape, rough, n_tab):
    L = gpu
    n_src, tile32, bord = shape
    assert mc.prefilter_table(L, rough)[1] > 1000
    tag = f"n_src {n_src} tile32 {tile32} rough {rough} n_tab {n_tab or 'full'}"
    on = _run(L, bord, rough, n_tab, tile32, 1)
    off = _run(L, bord, rough, n_tab, tile32, 0)
    if n_src > 64 and (n_tab or mc.prefilter_table(L, rough)[1]) == 8192:
        # 24 quarter-face regions x 256 mask words do not fit the kernel's LDS: launch_mc_region declines the level, another kernel
        # serves it and the switch has nothing to act on.  The case stays: no region launch, the same bytes.
        assert on[1].get("slices", 0) == 0 and off[1].get("slices", 0) == 0 and on[0] == off[0], tag
        return
    _check_pair(on, off, tag)
    # the ragged row windows of the other kernel-level tests, net off: those rows of the full dispatch
    full = np.frombuffer(on[0], np.float32).reshape(6, OUT, OUT, 4)
    for window in WINDOWS:
        data, c, took = _run(L, bord, rough, n_tab, tile32, 0, [window])
        win = np.frombuffer(data, np.float32).reshape(6, OUT, OUT, 4)
        f0, f1, y0, rows = window
        assert took == 0 and c["healed"] == 0 and c["count_only"] == 0 and c["slices"] > 0, (tag, window, took, c)
        assert win[f0:f1, y0:y0 + rows].tobytes() == full[f0:f1, y0:y0 + rows].tobytes(), (tag, window)


def test_condition_against_a_vacuous_pass(gpu):
    """128^2 -> 256^2, roughness 0.03, whole table: the checked kernel must absorb words AND walk count-only bodies, the two things the
    net-less kernel drops, or the comparison above shows nothing.  The stock level absorbs words (1.26 M wave-words) but every one of them
    is a word of the launch cut or fully proved: 0 count-only wave-samples.  So one 4 x 4 patch of it is scaled by 1e5: the level's maximum
    rises, the launch cut keeps more words, and the tiles far from the patch absorb them one by one (2.0 M count-only wave-samples)."""
    L = gpu
    lvl = level(128)
    lvl[4, 58:62, 58:62, :3] *= 1e5
    bord = mc.BorderedLevel(L, lvl)
    try:
        on = _run(L, bord, 0.03, None, 0, 1)
        off = _run(L, bord, 0.03, None, 0, 0)
    finally:
        bord.free()
    _check_pair(on, off, "128 -> 256^2, 0.03, a 4 x 4 patch scaled by 1e5")
    assert on[1]["abs_words"] > 0 and on[1]["count_only"] > 0, on[1]


def test_default_rule_follows_the_counters(gpu, shape):
    """The suite runs with PBR_MC_STATS=1: the rule (-1) keeps the net, so every healed == 0 of the other test files checks the real one."""
    n_src, tile32, bord = shape
    _, c, took = _run(gpu, bord, 0.03, 1000, tile32, -1)
    assert took == 1 and c["healed"] == 0 and c["slices"] > 0, (took, c)


@pytest.mark.parametrize("n_src,tile32", [(128, 0), (128, 1), (64, 0), (32, 0)], ids=lambda v: str(v))
def test_row_shards_and_single_faces(gpu, n_src, tile32):
    """Ragged row shards (three per face) and single faces with the net off: the full dispatch with the net off and with it on."""
    L = gpu
    bord = mc.BorderedLevel(L, level(n_src))
    try:
        on, _, t1 = _run(L, bord, 0.03, None, tile32, 1)
        off, _, t0 = _run(L, bord, 0.03, None, tile32, 0)
        assert (t1, t0) == (1, 0) and on == off
        for name, windows in (("shards", SHARDS), ("faces", SINGLE_FACES)):
            data, c, took = _run(L, bord, 0.03, None, tile32, 0, windows)
            assert took == 0 and c["healed"] == 0 and c["count_only"] == 0 and c["slices"] > 0, (name, took, c)
            assert data == off, name
    finally:
        bord.free()


def _hostile(kind):
    lvl = level(128)
    if kind == "negative":
        lvl[1, 30, 40, 0] = -1e9
    elif kind == "inf":
        lvl[3, 50, 20, 2] = np.inf
    elif kind == "black":
        lvl[..., 1] = 0.0
    else:
        lvl[4, 58:62, 58:62, :3] *= 1e5
    return lvl                                                         # every hostile texel lies inside [:64, :64]: the whole-face case crops


@pytest.mark.parametrize("kind", ["negative", "inf", "black", "bright"])
def test_hostile_texels(gpu, kind):
    """One negative texel and one infinite one (each switches the absorbed-word skip off for the regions that stage it), a black channel (a
    zero sum never absorbs) and a 1e5 : 1 patch: net off == net on, NaN and inf bytes included, on quarter faces with both tiles; the same
    four on the whole-face shape."""
    L = gpu
    for n_src, tile32 in ((128, 0), (128, 1), (64, 0)):
        lvl = _hostile(kind)
        if n_src == 64:
            lvl = np.ascontiguousarray(lvl[:, :64, :64])
        bord = mc.BorderedLevel(L, lvl)
        try:
            on = _run(L, bord, 0.03, None, tile32, 1)
            off = _run(L, bord, 0.03, None, tile32, 0)
        finally:
            bord.free()
        _check_pair(on, off, f"{kind} n_src {n_src} tile32 {tile32}")
        out = np.frombuffer(on[0], np.float32)
        if kind in ("negative", "inf"):
            assert not np.isfinite(out).all() or out.min() < 0, kind   # the texel reached the output
        if kind == "black":
            assert on[1]["abs_words"] == 0, on[1]


def _filter_table(L, bord, tab, alpha, tile32, net):
    """pbrk_mc_filter over the whole 256^2 cube with a table of the test's own: (bytes, counters, pbrk_mc_last_net())."""
    dtab = mc.DeviceBuffer(L, tab.nbytes, tab)
    zero = np.zeros((6, OUT, OUT, 4), np.float32)
    out = mc.DeviceBuffer(L, zero.nbytes, zero)
    try:
        with mc.switches(L, tile32=tile32, net=net):
            mc.reset_counters(L)
            rc = L.pbrk_mc_filter(bord.dev.ptr, None, bord.n_src, dtab.ptr, len(tab), float(np.pi), alpha, out.ptr, OUT, 0, 6, 0, OUT, None)
            assert rc == 0, rc
            data = out.read()
            return data, mc.counters(L, "skip", "flag", "window", "region", reset=True), L.pbrk_mc_last_net()
    finally:
        out.free()
        dtab.free()


@pytest.mark.parametrize("n_src,tile32", [(128, 0), (128, 1), (64, 0)], ids=lambda v: str(v))
def test_table_whose_word_maxima_rise_again(gpu, n_src, tile32):
    """The net-less kernel ends a pass at the first absorbed word behind which the slice's word maxima never rise (header 2l).  The
    reference's tables fall from their head words on; here the samples of word 2 and word 30 of the roughness-0.03 table change places, so
    slice 2 % S is monotone only from word 30 on and an absorbed word before it must not end the pass.  A 1e5 : 1 patch keeps words
    out of the launch cut.  Same bytes and absorbed counts as the checked kernel."""
    L = gpu
    tab = np.zeros((8192, 4), dtype=np.float32)
    alpha = C.c_float()
    n = L.pbrk_host_prefilter_table(8192, 0.03, tab.ctypes.data_as(C.c_void_p), C.byref(alpha))
    tab = np.ascontiguousarray(tab[:n])
    tab[64:96], tab[960:992] = tab[960:992].copy(), tab[64:96].copy()
    mono = (C.c_int * 4)()
    assert L.pbrk_mc_mono_slices(np.ascontiguousarray(tab[:, 3]).ctypes.data_as(C.POINTER(C.c_float)), n, 4, mono) == 0 and mono[2] == 30
    lvl = level(128)
    lvl[4, 58:62, 58:62, :3] *= 1e5
    bord = mc.BorderedLevel(L, np.ascontiguousarray(lvl[:, :n_src, :n_src]))
    try:
        on = _filter_table(L, bord, tab, alpha.value, tile32, 1)
        off = _filter_table(L, bord, tab, alpha.value, tile32, 0)
    finally:
        bord.free()
    _check_pair(on, off, f"words 2 and 30 swapped, n_src {n_src} tile32 {tile32}")
    assert on[1]["abs_words"] > 0, on[1]


def _chain(L, tex, net, mips):
    spec = pbrhip.make_texture(pbrhip.Format_RGBA32F, C4_S, C4_S, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps | pbrhip.TextureFlag_StorageImage)
    try:
        with mc.switches(L, net=net):
            mc.reset_counters(L)
            L.PBR_GenPrefilteredEnvMap(tex, spec, C4_MIN)
            L.GPU_WaitUntilIdle()
            c = mc.counters(L, "skip", "region", reset=True)
            return {m: mc.digest(pbrhip.read_mip(spec, m)) for m in mips}, c
    finally:
        L.GPU_DestroyTexture(spec)


def test_c4_at_full_size(gpu, c4_env):
    """C4 (2048^2 -> 4096^2): mip 1 takes the 32 x 32 tile on quarter faces, mip 2 whole faces, mip 3 the 34^2 shape.  Digests with the net
    off equal those with it on."""
    L = gpu
    tex = mc.env_texture(c4_env)
    try:
        on, c1 = _chain(L, tex, 1, (1, 2, 3))
        off, c0 = _chain(L, tex, 0, (1, 2, 3))
    finally:
        L.GPU_DestroyTexture(tex)
    print(f"C4: net 1 {c1}; net 0 {c0}")
    assert on == off
    assert c1["healed"] == 0 and c0["healed"] == 0 and c1["slices"] == c0["slices"] > 0
    assert c1["abs_words"] == c0["abs_words"] > 0 and c1["abs_samples"] == c0["abs_samples"]
    assert c1["count_only"] > 0 and c0["count_only"] == 0


def test_work_units(gpu, c4_env):
    """Ragged row shards and single faces as work units through PBR_RecordUnits, net off, on the quarter-face level 128^2 -> 256^2 (mip 1
    of a 512^2 cube from the C4 environment) and the whole-face and 34^2 levels of C4 (mips 2 and 3 of the 4096^2 cube): the whole-level
    unit with the net off and with it on."""
    L = gpu
    tex = mc.env_texture(c4_env)

    def run(S, mips, units, net):
        with mc.switches(L, net=net), mc.dispatch_prefilter_units(L, tex, S, units) as maps:
            took = L.pbrk_mc_last_net()
            c = mc.counters(L, "skip", "region", reset=True)
            assert took == net and c["healed"] == 0 and c["slices"] > 0 and (net or c["count_only"] == 0), (S, mips, net, took, c)
            return {m: mc.digest(pbrhip.read_mip(maps.tex_specular_env_map, m)) for m in mips}

    try:
        for S, mips in ((512, (1,)), (C4_S, (2, 3))):
            whole = [pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, m, 0, 6, 0, S >> m, 0.0) for m in mips]
            shards, faces = [], []
            for m in mips:
                size = S >> m
                for f in range(6):
                    cuts = (0, 5 + f, 131 - 2 * f, size)
                    shards += [pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, m, f, f + 1, cuts[k], cuts[k + 1], 0.0) for k in range(3)]
                    faces.append(pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, m, f, f + 1, 0, size, 0.0))
            on = run(S, mips, whole, 1)
            assert run(S, mips, whole, 0) == on, (S, "whole")
            assert run(S, mips, shards, 0) == on, (S, "shards")
            assert run(S, mips, faces, 0) == on, (S, "faces")
    finally:
        L.GPU_DestroyTexture(tex)
