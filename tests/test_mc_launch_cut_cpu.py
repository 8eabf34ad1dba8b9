"""The launch-level cut of the region kernel (k_mc_region.hip, header 2g; mc_launch_cut in k_mc_internal.h) through its host entry
pbrk_mc_launch_cut, checked exactly with fractions in the style of test_absorb_lemma_cpu.py:

  * every sample of a cut word leaves a lane's three fp32 sums unchanged, bit for bit, once the slice's head word has been
    accumulated -- taps anywhere in [m, M], the kernel's six tap weights and twelve FMAs;
  * the cut returned is the smallest one the stated inequality (evaluated in double, left to right) allows;
  * hostile inputs (m <= 0, subnormal m, negative / -0.0 weights, inf, NaN, tables of at most 128 samples) give no cut;
  * the levels the GPU tests generate give a non-trivial cut on both reference tables."""
import ctypes as C
from fractions import Fraction as F

import numpy as np
import pytest

from f32_exact import SC, bits, from_bits, mul, rnd, round_f32, to_int
from mc_cases import level
from mc_cut_ref import head_sum, run_sample

f32 = np.float32
ROUGH = (0.03, 0.15)                                          # the tables of C4 mip 1 (1389 samples) and mip 2 (8192)
# (m, M): ratios from 1 to 1e6
RANGES = [(1.0, 1.0), (0.1, 1.1), (0.37, 25.0), (1e-3, 1.0), (0.01, 1e3), (2.5e-4, 250.0), (1.0, 1e6)]


def test_integer_rounding_is_the_fraction_rounding():
    rng = np.random.default_rng(2)
    for _ in range(400):
        a = float(f32(rng.uniform(0, 1) * 2.0 ** int(rng.integers(-60, 20))))
        b = float(f32(rng.uniform(0, 1) * 2.0 ** int(rng.integers(-60, 20))))
        c = float(f32(rng.uniform(0, 1) * 2.0 ** int(rng.integers(-100, 30))))
        want = round_f32(F(a) * F(b) + F(c))
        assert F(rnd(mul(to_int(a), to_int(b)) + to_int(c)), 2 ** SC) == want
        assert F(rnd(to_int(c)), 2 ** SC) == F(c)
    assert rnd(to_int(2.0 ** -149) >> 1) == 0                 # a tie at half the smallest subnormal rounds to even


@pytest.fixture(scope="module")
def L():
    import pbrhip
    return pbrhip.lib()                                       # binds the symbols; no GPU call


@pytest.fixture(scope="module")
def tables(L):
    out = {}
    for rough in ROUGH:
        tab = np.zeros((8192, 4), dtype=np.float32)
        alpha = C.c_float()
        n = L.pbrk_host_prefilter_table(8192, rough, tab.ctypes.data_as(C.c_void_p), C.byref(alpha))
        assert 128 < n <= 8192
        out[rough] = tab[:n].copy()
    return out


def lib_cut(L, w, m_bits, M_bits):
    w = np.ascontiguousarray(w, dtype=np.float32)
    cut4 = (C.c_int * 4)()
    k = L.pbrk_mc_launch_cut(w.ctypes.data_as(C.POINTER(C.c_float)), len(w), m_bits, M_bits, cut4)
    return k, list(cut4)


def slice_end(s, NW):
    return s if s >= NW else s + 4 * ((NW - s + 3) // 4)


def word_ok(w, wd, s, m, M):
    """The stated inequality for word wd of slice s, in double, left to right."""
    W = float(np.max(w[32 * wd:32 * wd + 32]))
    return W * M * 2.0 ** 25 * (1.0 + 2.0 ** -10) <= head_sum(w, s) * m


def expected_cut(w, m, M):
    NW = (len(w) + 31) // 32
    cut = [slice_end(s, NW) for s in range(4)]
    for s in range(4):
        if not head_sum(w, s) * m * 2.0 ** -25 >= 2.0 ** -100:
            continue
        c = cut[s]
        while c - 4 > s and word_ok(w, c - 4, s, m, M):
            c -= 4
        cut[s] = c
    return cut


# ---- smallest cut -----------------------------------------------------------------------------

@pytest.mark.parametrize("rough", ROUGH)
def test_cut_is_the_smallest_the_inequality_allows(L, tables, rough):
    w = tables[rough][:, 3]
    NW = (len(w) + 31) // 32
    for m, M in RANGES:
        m, M = float(f32(m)), float(f32(M))
        k, cut = lib_cut(L, w, bits(m), bits(M))
        assert cut == expected_cut(w, m, M), (m, M)
        assert k == sum((slice_end(s, NW) - cut[s]) // 4 for s in range(4)) and k > 0, (m, M, cut)
        for s in range(4):
            assert cut[s] % 4 == s and s < cut[s] <= slice_end(s, NW)
            for wd in range(cut[s], NW, 4):
                assert word_ok(w, wd, s, m, M)                  # every word at or behind the cut satisfies it
            if cut[s] - 4 > s:
                assert not word_ok(w, cut[s] - 4, s, m, M)      # one word earlier violates it
            # the head word itself is never cut
            assert cut[s] >= s + 4


@pytest.mark.parametrize("rough", ROUGH)
def test_cut_on_the_boundary_of_the_inequality(L, tables, rough):
    """m chosen so that one word sits on the boundary: the cut moves between m and its fp32 neighbours exactly as the double
    evaluation says."""
    w = tables[rough][:, 3]
    NW = (len(w) + 31) // 32
    moved = 0
    for M in (1.0, 37.5, 1e4):
        for s in range(4):
            for wd in (s + 4, s + 4 * ((NW // 4) // 2), slice_end(s, NW) - 4):
                W = float(np.max(w[32 * wd:32 * wd + 32]))
                if W == 0.0:
                    continue
                m0 = f32(W * M * 2.0 ** 25 * (1.0 + 2.0 ** -10) / head_sum(w, s))
                if not (1e-30 < float(m0) < 1e30):
                    continue
                cuts = []
                for mb in (bits(m0) - 2, bits(m0) - 1, bits(m0), bits(m0) + 1, bits(m0) + 2):
                    m = from_bits(mb)
                    k, cut = lib_cut(L, w, mb, bits(M))
                    assert cut == expected_cut(w, m, float(f32(M))), (M, s, wd, mb)
                    cuts.append(cut[s])
                assert cuts == sorted(cuts, reverse=True)       # a larger m never cuts less
                moved += cuts[0] != cuts[-1]
    assert moved > 0, "no case straddled the boundary: the cases check nothing"


# ---- no-op chain ------------------------------------------------------------------------------

def chain_case(L, w, m, M, s, rng, reverse_head=False, grow_tail=False):
    m, M = float(f32(m)), float(f32(M))
    Fm, FM = to_int(m), to_int(M)
    k, cut = lib_cut(L, w, bits(m), bits(M))
    NW = (len(w) + 31) // 32
    assert cut[s] < slice_end(s, NW), "nothing cut: the case checks nothing"
    mid = to_int(f32(rng.uniform(m, M)))
    unit = lambda: to_int(f32(rng.uniform(0, 1)))             # a, b in [0, 1)
    head = list(range(32 * s, 32 * s + 32))
    if reverse_head:
        head.reverse()
    acc = [0, 0, 0]
    for i in head:
        # R: every tap at m (the smallest sums a lane can reach); G: random taps in [m, M]; B: every tap at M
        g = [to_int(f32(rng.uniform(m, M))) for _ in range(4)]
        acc = run_sample(acc, to_int(w[i]), unit(), unit(), ([Fm] * 4, g, [FM] * 4))
    if grow_tail:                                             # the uncut tail words first, as a tile would; the sums only grow
        for wd in range(s + 4, cut[s], 4):
            for i in range(32 * wd, 32 * wd + 32, 5):
                acc = run_sample(acc, to_int(w[i]), to_int(0.5), to_int(0.25), ([Fm] * 4, [mid] * 4, [FM] * 4))
    assert all(F(x, 2 ** SC) >= F(2) ** -100 for x in acc)
    for wd in range(cut[s], NW, 4):
        for i in range(32 * wd, min(32 * wd + 32, len(w))):
            wgt = to_int(w[i])
            # the worst case: the whole weight on one tap at M (a = b = 0), in every sum; then random a, b
            for a, b in ((0, 0), (unit(), unit())):
                assert run_sample(acc, wgt, a, b, ([FM] * 4,) * 3) == acc, (m, M, s, wd, i)


@pytest.mark.parametrize("rough", ROUGH)
def test_cut_words_are_no_ops_after_the_head_word(L, tables, rough):
    w = tables[rough][:, 3]
    rng = np.random.default_rng(5)
    for k, (m, M) in enumerate(RANGES):
        chain_case(L, w, m, M, k % 4, rng, reverse_head=bool(k & 1), grow_tail=(k % 3 == 2))
    for s in range(4):                                        # every slice once, on the range of the generated levels
        chain_case(L, w, 0.1, 1.1, s, rng)


def test_no_op_chain_on_the_boundary(L, tables):
    """m on the boundary of the last uncut word of slice 1: the words behind it are still exact no-ops."""
    w = tables[0.03][:, 3]
    rng = np.random.default_rng(9)
    M = 3.0
    _, cut = lib_cut(L, w, bits(0.5), bits(M))
    wd = cut[1]
    W = float(np.max(w[32 * wd:32 * wd + 32]))
    m0 = f32(W * M * 2.0 ** 25 * (1.0 + 2.0 ** -10) / head_sum(w, 1))
    for mb in (bits(m0), bits(m0) + 1):
        chain_case(L, w, from_bits(mb), M, 1, rng)


# ---- hostile inputs ---------------------------------------------------------------------------

def assert_no_cut(L, w, m_bits, M_bits):
    NW = (len(w) + 31) // 32
    k, cut = lib_cut(L, w, m_bits, M_bits)
    assert k == 0 and cut == [slice_end(s, NW) for s in range(4)], (k, cut)


@pytest.mark.parametrize("rough", ROUGH)
def test_no_cut_on_hostile_inputs(L, tables, rough):
    w = tables[rough][:, 3].copy()
    one = bits(1.0)
    assert lib_cut(L, w, one, one)[0] > 0
    for mb in (bits(0.0), bits(-0.0), bits(-1.0), 1, 0x007fffff, bits(np.inf), bits(np.nan)):      # zero, negative, subnormal, inf, NaN
        assert_no_cut(L, w, mb, one)
    for Mb in (bits(np.inf), bits(np.nan), bits(-1.0), bits(-0.0)):
        assert_no_cut(L, w, one, Mb)
    for pos in (0, 40, 200, len(w) - 1):
        for bad in (-1e-9, -0.0, np.inf, np.nan):
            v = w.copy()
            v[pos] = bad
            assert_no_cut(L, v, one, one)
    for n in (1, 31, 32, 100, 128):                           # one phase: no tail to cut
        assert_no_cut(L, w[:n], one, one)
    assert lib_cut(L, w[:129], one, one)[1][0] in (4, 8)      # 129 samples: a tail exists (cut or not, by the inequality)
    # sums too small for the lemma's normal range: H m 2^-25 < 2^-100
    assert_no_cut(L, w, bits(1e-30), bits(1e-30))


def test_bad_arguments(L, tables):
    w = np.ascontiguousarray(tables[0.03][:, 3])
    cut4 = (C.c_int * 4)()
    p = w.ctypes.data_as(C.POINTER(C.c_float))
    assert L.pbrk_mc_launch_cut(None, 10, 1, 1, cut4) == -1
    assert L.pbrk_mc_launch_cut(p, 0, 1, 1, cut4) == -1
    assert L.pbrk_mc_launch_cut(p, 8193, 1, 1, cut4) == -1
    assert L.pbrk_mc_launch_cut(p, 10, 1, 1, None) == -1


# ---- the generator's own inputs ---------------------------------------------------------------

@pytest.mark.parametrize("n_src,rough", [(128, 0.03), (64, 0.15), (100, 0.03), (48, 0.15)])
def test_generated_levels_give_a_cut(L, tables, n_src, rough):
    """The levels of tests/test_gpu_mc_launch_cut.py (mc_cases.level): every texel of the bordered level is a texel of the level (or a mean of such), so
    the level's own extrema bound the cut from the safe side.  The bright patch moves the cut later and leaves one."""
    w = tables[rough][:, 3]
    NW = (len(w) + 31) // 32
    lvl = level(n_src)[..., :3]
    k, cut = lib_cut(L, w, bits(lvl.min()), bits(lvl.max()))
    assert k >= NW // 4, (k, NW)
    kb, cutb = lib_cut(L, w, bits(lvl.min()), bits(lvl.max() * f32(1e5)))
    assert 0 < kb < k and all(b > a for a, b in zip(cut, cutb))
