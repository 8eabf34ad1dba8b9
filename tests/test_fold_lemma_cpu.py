"""The lemma behind the folded frame rows of the region kernel (k_mc_region.hip, header 2j), in exact arithmetic: with half_n = 2^k
multiplied into the sc and tc rows of the permuted frame, the three-FMA chain returns 2^k times what it returned, bit for bit; the
tap coordinate fma(sc', rcp(ma), off) is the one of fma(sc, rcp(ma) 2^k, off); and the in-face tests decide on (sc', tc', ma 2^k) as
they did on (sc, tc, ma).  Condition: no non-zero intermediate below 2^-126 and none at or above 2^128 -- the last test shows what
a subnormal does to it.  Signed zeros: a Fraction has one zero; -0 compares and adds like +0 in every step checked here, and the
inputs below hold both.  No GPU."""
from fractions import Fraction as F

import numpy as np
import pytest

from f32_exact import round_f32

N_CASES = 1500
KS = (3, 4, 5, 6)                                                  # half_n 8 .. 64: source levels 16 .. 128


def fma(a, b, c):
    return round_f32(a * b + c)


def chain(e, pb, pt, pr):
    """to_face's row: fma(e.x, Pb, fma(e.y, Pt, e.z * Pr))"""
    return fma(e[0], pb, fma(e[1], pt, round_f32(e[2] * pr)))


def on_face(cls, sc, tc, ma):
    """on_face<CLS> of the kernel: the hardware's tie rule in two comparisons"""
    if cls == 0:
        return ma > abs(sc), ma > abs(tc)
    if cls == 1:
        return ma >= abs(sc), ma > abs(tc)
    return ma >= abs(sc), ma >= abs(tc)


def f32(v):
    return F(float(np.float32(v)))


def _cases():
    """(entry, sc row, tc row, ma row) as exact fp32 values: unit local directions and frame rows in [-1, 1], with components that
    are exactly 0 or -0, as small as the kernel ever meets (1e-8), and rows that tie the in-face comparisons"""
    rng = np.random.default_rng(0xF01D)
    special = [0.0, -0.0, 1e-8, -1e-8, 1.0, -1.0, 0.5]
    out = []
    for i in range(N_CASES):
        e = rng.normal(size=3)
        e /= np.linalg.norm(e)
        rows = rng.uniform(-1.0, 1.0, size=(3, 3))                 # [sc, tc, ma] x [Pb, Pt, Pr]
        if i % 3 == 0:
            for _ in range(rng.integers(1, 4)):
                rows[rng.integers(3), rng.integers(3)] = special[rng.integers(len(special))]
        if i % 5 == 0:
            e[rng.integers(3)] = special[rng.integers(2)]          # 0 or -0
        if i % 7 == 0:
            rows[2] = rows[0] if i % 2 else -rows[1]               # ma row = the sc row / minus the tc row: exact ties
        out.append(([f32(v) for v in e], [[f32(v) for v in r] for r in rows], int(rng.integers(1 << 30))))
    return out


CASES = _cases()


@pytest.mark.parametrize("k", KS)
def test_scaled_rows_scale_the_chain_and_keep_every_decision(k):
    h = F(2) ** k
    ties = taps = 0
    for e, (rs, rt, rm), seed in CASES:
        sc, tc, ma = chain(e, *rs), chain(e, *rt), chain(e, *rm)
        for row in (rs, rt):
            assert all(round_f32(v * h) == v * h for v in row)     # the six multiplies of a staging are exact
        scs, tcs = chain(e, *[v * h for v in rs]), chain(e, *[v * h for v in rt])
        # 1. the chain commutes with the scaling, bit for bit
        assert scs == h * sc and tcs == h * tc, (e, rs, rt, k)
        # 2. the in-face tests: ma half_n is exact, and all three classes decide as before
        mas = round_f32(ma * h)
        assert mas == ma * h
        for cls in (0, 1, 2):
            assert on_face(cls, scs, tcs, mas) == on_face(cls, sc, tc, ma), (cls, e, rs, rt, rm, k)
        ties += ma == abs(sc) or ma == abs(tc)
        # 3. the tap coordinates, with any fp32 reciprocal (v_rcp_f32 is good to an ulp: take the rounded one and a neighbour)
        if ma > 0:
            r = round_f32(1 / ma)
            r += (seed % 3 - 1) * (r / 2 ** 23 if seed % 2 else 0)
            r = round_f32(r)
            assert round_f32(r * h) == r * h                       # the multiply the proved body loses was exact
            off = h + F(1, 2)                                      # 0.5 n + 0.5
            assert fma(scs, r, off) == fma(sc, r * h, off) and fma(tcs, r, off) == fma(tc, r * h, off)
            taps += 1
    assert taps > N_CASES // 3 and ties > 0, (taps, ties)          # the cases meet what they are meant to check


def test_a_subnormal_product_is_where_the_lemma_ends():
    """Why the header states a condition: 1.5 x 2^-149 rounds to 2 x 2^-149 (ties to even), eight times that is 16 x 2^-149, but the
    scaled row gives 12 x 2^-149 exactly.  The kernel's rows and entries are 0 or at least ~1e-8 in magnitude: no product comes near."""
    tiny = F(3, 2 ** 149)
    e = [F(1, 2), F(0), F(0)]
    plain = chain(e, tiny, F(0), F(0))
    scaled = chain(e, tiny * 8, F(0), F(0))
    assert plain == F(2, 2 ** 149) and scaled == F(12, 2 ** 149) and scaled != 8 * plain
    # and what such a miss can be at most: a term of subnormal size, far below the ulp of any sum a comparison or a tap can see
    assert abs(scaled - 8 * plain) < F(1, 2 ** 126) * 8
