"""pbrk_mc_mono_slices, the host twin of what k_mc_cut writes for the net-less region kernel's early end of a pass (k_mc_region.hip, header
2l; mc_mono_from in k_mc_internal.h), against numpy.  Slice s of S owns the mask words s, s + S, ..; mono[s] is the first of them from
which the slice's word maxima (the largest weight of each word of 32 samples, compared as bit patterns) never rise again.  No GPU."""
import ctypes as C

import numpy as np
import pytest

SLICES = (1, 4)
LENGTHS = (1, 33, 8192)


@pytest.fixture(scope="module")
def L():
    import pbrhip
    return pbrhip.lib()                                       # binds the symbols; no GPU call


def lib_mono(L, w, S):
    w = np.ascontiguousarray(w, dtype=np.float32)
    mono = (C.c_int * 4)(-7, -7, -7, -7)
    assert L.pbrk_mc_mono_slices(w.ctypes.data_as(C.POINTER(C.c_float)), len(w), S, mono) == 0
    assert list(mono)[S:] == [-7] * (4 - S)                   # S entries are written
    return list(mono)[:S]


def ref_mono(w, S):
    """Straight from the definition: the smallest word k of the slice such that no later pair of consecutive words of the slice rises."""
    w = np.asarray(w, dtype=np.float32)
    nw = (len(w) + 31) // 32
    wmax = [int(w[32 * k:32 * k + 32].view(np.uint32).max()) for k in range(nw)]
    out = []
    for s in range(S):
        words = list(range(s, nw, S))
        k = s
        for j in range(len(words)):
            if all(wmax[words[i + 1]] <= wmax[words[i]] for i in range(j, len(words) - 1)):
                k = words[j]
                break
        out.append(k)
    return out


def prefilter_weights(L, rough):
    tab = np.zeros((8192, 4), dtype=np.float32)
    alpha = C.c_float()
    n = L.pbrk_host_prefilter_table(8192, rough, tab.ctypes.data_as(C.c_void_p), C.byref(alpha))
    assert 0 < n <= 8192
    return tab[:n, 3].copy()


def irradiance_weights(L):
    tab = np.zeros((8192, 4), dtype=np.float32)
    L.pbrk_host_irradiance_table(8192, tab.ctypes.data_as(C.c_void_p))
    return tab[:, 3].copy()


@pytest.mark.parametrize("S", SLICES)
@pytest.mark.parametrize("rough", [0.03, 0.15, 0.4, 0.6, None], ids=lambda r: "irradiance" if r is None else f"r{r}")
def test_reference_tables_are_monotone_from_word_0(L, rough, S):
    """The reference's tables take their samples in order of rising pitch: every slice's maxima fall from its head word on, so the first
    absorbed word of a pass ends it."""
    w = irradiance_weights(L) if rough is None else prefilter_weights(L, rough)
    got = lib_mono(L, w, S)
    assert got == ref_mono(w, S)
    assert got == list(range(S)), (rough, S, got)


@pytest.mark.parametrize("S", SLICES)
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(L, n, S):
    """One sample (one ragged word; with four slices three of them own no word and get their own index), 33 (two words, the last ragged) and
    8192 (256 words), each a prefix of the roughness-0.15 table and of a table of random weights."""
    rng = np.random.default_rng(n + S)
    for w in (prefilter_weights(L, 0.15)[:n], rng.random(n, dtype=np.float32)):
        assert len(w) == n
        assert lib_mono(L, w, S) == ref_mono(w, S), (n, S)
    if n == 1:
        assert lib_mono(L, np.ones(1, np.float32), S) == list(range(S))


@pytest.mark.parametrize("S", SLICES)
def test_one_raised_weight_in_word_9(L, S):
    """Word 9 belongs to slice 9 % S; raised above the word before it in that slice, the slice is monotone from word 9 on and no earlier.
    The other slices stay monotone from their head."""
    w = prefilter_weights(L, 0.03)
    w[9 * 32 + 5] = w[:32].max() * 2.0
    got = lib_mono(L, w, S)
    assert got == ref_mono(w, S)
    want = list(range(S))
    want[9 % S] = 9
    assert got == want, (S, got)


def test_bad_arguments(L):
    w = np.ones(64, np.float32)
    mono = (C.c_int * 4)()
    p = w.ctypes.data_as(C.POINTER(C.c_float))
    assert L.pbrk_mc_mono_slices(p, 64, 3, mono) == -1
    assert L.pbrk_mc_mono_slices(p, 0, 4, mono) == -1
    assert L.pbrk_mc_mono_slices(p, 8193, 4, mono) == -1
    assert L.pbrk_mc_mono_slices(None, 64, 4, mono) == -1
