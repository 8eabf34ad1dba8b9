"""The launch-level cut for S slices per workgroup (k_mc_region.hip, header 2h; mc_launch_cut_s in k_mc_internal.h) through its host
entry pbrk_mc_launch_cut_slices, checked exactly with fractions with the helpers of f32_exact.py and mc_cut_ref.py.  Slice s of S owns the
mask words s, s + S, ..; word s is its head.  S = 4 is the 16 x 16 tile's cut (pbrk_mc_launch_cut), S = 1 the 32 x 32 tile's: one
head word, weighed against the whole table.

  * the cut returned is the smallest one the stated inequality (in double, left to right) allows, for S = 1, 2, 4 and tables of 33,
    64, 1389 and 2048 samples;
  * S = 4 equals pbrk_mc_launch_cut on every case, the hostile ones included;
  * hostile inputs (subnormal minimum, inf, a negative weight, NW <= S) give no cut;
  * every sample of a cut word leaves a lane's three fp32 sums unchanged, bit for bit, for sums at the proved lower bound -- the
    slice's head word accumulated with every tap at m."""
import ctypes as C
from fractions import Fraction as F

import numpy as np
import pytest

from f32_exact import SC, bits, from_bits, to_int
from mc_cut_ref import head_sum, run_sample

f32 = np.float32

SLICES = (1, 2, 4)
# (roughness of the reference's table, samples taken from its front): 1389 is the whole roughness-0.03 table (C4 mip 1); 2048 samples
# are the longest table the one-slice tile serves (64 mask words)
TABLES = [(0.03, 33), (0.03, 64), (0.03, 1389), (0.04, 2048)]
RANGES = [(1.0, 1.0), (0.1, 1.1), (0.37, 25.0), (1e-3, 1.0), (0.01, 1e3), (2.5e-4, 250.0), (1.0, 1e6)]


@pytest.fixture(scope="module")
def L():
    import pbrhip
    return pbrhip.lib()                                       # binds the symbols; no GPU call


@pytest.fixture(scope="module")
def weights(L):
    out = {}
    for rough, n in TABLES:
        tab = np.zeros((8192, 4), dtype=np.float32)
        alpha = C.c_float()
        k = L.pbrk_host_prefilter_table(8192, rough, tab.ctypes.data_as(C.c_void_p), C.byref(alpha))
        assert n <= k <= 8192
        out[(rough, n)] = tab[:n, 3].copy()
    assert len(out[(0.03, 1389)]) == 1389
    return out


def lib_cut_s(L, w, S, m_bits, M_bits):
    w = np.ascontiguousarray(w, dtype=np.float32)
    cut = (C.c_int * 4)(-7, -7, -7, -7)
    k = L.pbrk_mc_launch_cut_slices(w.ctypes.data_as(C.POINTER(C.c_float)), len(w), S, m_bits, M_bits, cut)
    assert list(cut)[S:] == [-7] * (4 - S)                    # S entries are written
    return k, list(cut)[:S]


def lib_cut4(L, w, m_bits, M_bits):
    w = np.ascontiguousarray(w, dtype=np.float32)
    cut = (C.c_int * 4)()
    k = L.pbrk_mc_launch_cut(w.ctypes.data_as(C.POINTER(C.c_float)), len(w), m_bits, M_bits, cut)
    return k, list(cut)


def slice_end(s, NW, S):
    return s if s >= NW else s + S * ((NW - s + S - 1) // S)


def word_ok(w, wd, s, m, M):
    """The stated inequality for word wd of slice s, in double, left to right."""
    W = float(np.max(w[32 * wd:32 * wd + 32]))
    return W * M * 2.0 ** 25 * (1.0 + 2.0 ** -10) <= head_sum(w, s) * m


def expected_cut(w, S, m, M):
    NW = (len(w) + 31) // 32
    cut = [slice_end(s, NW, S) for s in range(S)]
    if NW <= S:
        return cut
    for s in range(S):
        if not head_sum(w, s) * m * 2.0 ** -25 >= 2.0 ** -100:
            continue
        c = cut[s]
        while c - S > s and word_ok(w, c - S, s, m, M):
            c -= S
        cut[s] = c
    return cut


# ---- smallest cut; S = 4 is pbrk_mc_launch_cut -------------------------------------------------

@pytest.mark.parametrize("S", SLICES)
@pytest.mark.parametrize("table", TABLES)
def test_cut_is_the_smallest_the_inequality_allows(L, weights, table, S):
    w = weights[table]
    NW = (len(w) + 31) // 32
    for m, M in RANGES:
        m, M = float(f32(m)), float(f32(M))
        k, cut = lib_cut_s(L, w, S, bits(m), bits(M))
        assert cut == expected_cut(w, S, m, M), (m, M)
        assert k == sum((slice_end(s, NW, S) - cut[s]) // S for s in range(S)), (m, M, cut)
        if len(w) >= 1389:
            assert k > 0, (m, M, "nothing cut: the case checks nothing")
        for s in range(S):
            if s >= NW:
                assert cut[s] == s
                continue
            assert cut[s] % S == s and s + S <= cut[s] <= slice_end(s, NW, S)      # the head word itself is never cut
            for wd in range(cut[s], NW, S):
                assert word_ok(w, wd, s, m, M)                # every word at or behind the cut satisfies it
            if cut[s] - S > s:
                assert not word_ok(w, cut[s] - S, s, m, M)    # one word earlier violates it
        if S == 4:
            assert (k, cut) == lib_cut4(L, w, bits(m), bits(M))


def test_one_slice_cut_on_the_boundary_of_the_inequality(L, weights):
    """m chosen so that one word sits on the boundary: the cut moves between m and its fp32 neighbours as the double evaluation says."""
    moved = 0
    for table in ((0.03, 1389), (0.04, 2048)):
        w = weights[table]
        NW = (len(w) + 31) // 32
        for S in SLICES:
            for M in (1.0, 37.5):
                for wd in (S, S * (NW // S // 2), slice_end(0, NW, S) - S):
                    W = float(np.max(w[32 * wd:32 * wd + 32]))
                    if W == 0.0:
                        continue
                    m0 = f32(W * M * 2.0 ** 25 * (1.0 + 2.0 ** -10) / head_sum(w, 0))
                    if not (1e-30 < float(m0) < 1e30):
                        continue
                    cuts = []
                    for mb in range(bits(m0) - 2, bits(m0) + 3):
                        _, cut = lib_cut_s(L, w, S, mb, bits(M))
                        assert cut == expected_cut(w, S, from_bits(mb), float(f32(M))), (table, S, M, wd, mb)
                        cuts.append(cut[0])
                    assert cuts == sorted(cuts, reverse=True)   # a larger m never cuts less
                    moved += cuts[0] != cuts[-1]
    assert moved > 0, "no case straddled the boundary: the cases check nothing"


# ---- hostile inputs ---------------------------------------------------------------------------

def assert_no_cut(L, w, S, m_bits, M_bits):
    NW = (len(w) + 31) // 32
    k, cut = lib_cut_s(L, w, S, m_bits, M_bits)
    assert k == 0 and cut == [slice_end(s, NW, S) for s in range(S)], (S, k, cut)
    if S == 4:
        assert (k, cut) == lib_cut4(L, w, m_bits, M_bits)


@pytest.mark.parametrize("S", SLICES)
@pytest.mark.parametrize("table", [(0.03, 1389), (0.04, 2048)])
def test_no_cut_on_hostile_inputs(L, weights, table, S):
    w = weights[table].copy()
    one = bits(1.0)
    assert lib_cut_s(L, w, S, one, one)[0] > 0
    for mb in (bits(0.0), bits(-0.0), bits(-1.0), 1, 0x007fffff, bits(np.inf), bits(np.nan)):      # zero, negative, subnormal, inf, NaN
        assert_no_cut(L, w, S, mb, one)
    for Mb in (bits(np.inf), bits(np.nan), bits(-1.0), bits(-0.0)):
        assert_no_cut(L, w, S, one, Mb)
    for pos in (0, 40, 200, len(w) - 1):
        for bad in (-1e-9, -0.0, np.inf, np.nan):
            v = w.copy()
            v[pos] = bad
            assert_no_cut(L, v, S, one, one)
    for n in (1, 31, 32 * S - 1, 32 * S):                     # NW <= S: one phase, no tail to cut
        assert_no_cut(L, w[:n], S, one, one)
    k, cut = lib_cut_s(L, w[:32 * S + 1], S, one, one)        # one sample more: slice 0 has a tail (cut or not, by the inequality)
    assert cut[0] in (S, 2 * S) and k == (2 * S - cut[0]) // S
    # sums too small for the lemma's normal range: H m 2^-25 < 2^-100
    assert_no_cut(L, w, S, bits(1e-30), bits(1e-30))


def test_bad_arguments(L, weights):
    w = np.ascontiguousarray(weights[(0.03, 1389)])
    cut = (C.c_int * 4)()
    p = w.ctypes.data_as(C.POINTER(C.c_float))
    assert L.pbrk_mc_launch_cut_slices(None, 10, 1, 1, 1, cut) == -1
    assert L.pbrk_mc_launch_cut_slices(p, 0, 1, 1, 1, cut) == -1
    assert L.pbrk_mc_launch_cut_slices(p, 8193, 1, 1, 1, cut) == -1
    assert L.pbrk_mc_launch_cut_slices(p, 10, 1, 1, 1, None) == -1
    for S in (0, 3, 5, 8, -1):
        assert L.pbrk_mc_launch_cut_slices(p, len(w), S, bits(1.0), bits(1.0), cut) == -1


# ---- no-op chain ------------------------------------------------------------------------------

def chain_case(L, w, S, m, M, s, rng, reverse_head=False):
    """The head word of slice s accumulated with every R tap at m (the proved lower bound of a lane's sums), random G taps in [m, M]
    and every B tap at M; then every sample of every cut word of the slice, with its whole weight on one tap at M and with random
    fractions, must return the three sums unchanged."""
    m, M = float(f32(m)), float(f32(M))
    Fm, FM = to_int(m), to_int(M)
    _, cut = lib_cut_s(L, w, S, bits(m), bits(M))
    NW = (len(w) + 31) // 32
    assert cut[s] < slice_end(s, NW, S), "nothing cut: the case checks nothing"
    unit = lambda: to_int(f32(rng.uniform(0, 1)))             # a, b in [0, 1)
    head = list(range(32 * s, 32 * s + 32))
    if reverse_head:
        head.reverse()
    acc = [0, 0, 0]
    for i in head:
        g = [to_int(f32(rng.uniform(m, M))) for _ in range(4)]
        acc = run_sample(acc, to_int(w[i]), unit(), unit(), ([Fm] * 4, g, [FM] * 4))
    assert all(F(x, 2 ** SC) >= F(2) ** -100 for x in acc)
    for wd in range(cut[s], NW, S):
        for i in range(32 * wd, min(32 * wd + 32, len(w))):
            wgt = to_int(w[i])
            for a, b in ((0, 0), (unit(), unit())):
                assert run_sample(acc, wgt, a, b, ([FM] * 4,) * 3) == acc, (S, m, M, s, wd, i)


@pytest.mark.parametrize("S", SLICES)
@pytest.mark.parametrize("table", [(0.03, 1389), (0.04, 2048)])
def test_cut_words_are_no_ops_after_the_head_word(L, weights, table, S):
    w = weights[table]
    rng = np.random.default_rng(5)
    for k, (m, M) in enumerate(RANGES):
        chain_case(L, w, S, m, M, k % S, rng, reverse_head=bool(k & 1))
    for s in range(S):                                        # every slice once, on the range of the generated levels
        chain_case(L, w, S, 0.1, 1.1, s, rng)


def test_no_op_chain_on_the_boundary(L, weights):
    """One slice, m on the boundary of the first cut word: the words from it on are still exact no-ops."""
    w = weights[(0.03, 1389)]
    rng = np.random.default_rng(9)
    M = 3.0
    _, cut = lib_cut_s(L, w, 1, bits(0.5), bits(M))
    W = float(np.max(w[32 * cut[0]:32 * cut[0] + 32]))
    m0 = f32(W * M * 2.0 ** 25 * (1.0 + 2.0 ** -10) / head_sum(w, 0))
    for mb in (bits(m0), bits(m0) + 1):
        chain_case(L, w, 1, from_bits(mb), M, 0, rng)
