"""The lemma behind the region kernel's absorbed words (k_mc_region.hip, absorb_threshold), checked exactly with fractions:

    acc normal, positive; 0 <= x <= acc * 2^-25  =>  fl(acc + x) == acc   (one rounding, to nearest even, as in an fp32 FMA)

and the kernel's fp32 form of the test: acc >= max(fl(fl(fl(W M) (1 + 2^-20)) 2^25), 2^-100) implies W M <= acc 2^-25 exactly."""
from fractions import Fraction as F

import numpy as np

from f32_exact import round_f32

f32 = np.float32
TWO_M25 = F(1, 2 ** 25)


def fma_f32(x, y, acc):
    return round_f32(F(x) * F(y) + F(acc))


def f(v):
    return F(float(f32(v)))


def next_up(v):
    return f(np.nextafter(f32(v), f32(np.inf)))


def test_round_f32_matches_numpy():
    rng = np.random.default_rng(1)
    for v in rng.standard_normal(300) * 10.0 ** rng.integers(-30, 30, 300):
        assert round_f32(F(float(v))) == F(float(f32(v)))


def _check(acc, x):
    """x exact (a product w * q, any rational) with 0 <= x <= acc 2^-25: the FMA leaves acc unchanged."""
    assert 0 <= x <= acc * TWO_M25
    assert round_f32(acc + x) == acc


def test_lemma_boundary_powers_of_two_and_ties():
    for e in (-125, -100, -60, -1, 0, 1, 23, 24, 60, 127):
        acc = F(2) ** e
        _check(acc, acc * TWO_M25)                           # the boundary itself
        _check(acc, F(0))
        top = f(np.nextafter(f32(2.0 ** (e + 1) if e < 127 else np.inf), f32(0)))   # the largest float below 2^(e+1)
        _check(top, top * TWO_M25)
        # just past the bound the claim may fail: acc + ulp/2 is a tie that rounds away from an odd acc
        odd = f(np.nextafter(f32(2.0 ** e), f32(np.inf)))    # mantissa ...01: odd
        ulp = next_up(float(odd)) - odd
        assert round_f32(odd + ulp / 2) != odd                 # a tie from an odd mantissa moves: the lemma needs 2^-25, not 2^-24
        _check(odd, odd * TWO_M25)


def test_lemma_random_products():
    rng = np.random.default_rng(7)
    for _ in range(3000):
        acc = f(rng.uniform(1.0, 2.0) * 2.0 ** int(rng.integers(-120, 120)))
        # a product of two floats (weight x texel) up to the bound, and the bound itself
        w = f(rng.uniform(0.0, 1.0) * 2.0 ** int(rng.integers(-40, 0)))
        qmax = acc * TWO_M25 / w if w > 0 else F(1)
        q = f(min(float(qmax), 1e38) * rng.uniform(0.0, 1.0))    # a finite fp32 texel
        if F(w) * q <= acc * TWO_M25:
            _check(acc, F(w) * q)
        _check(acc, acc * TWO_M25 * F(int(rng.integers(0, 1000)), 1000))


def test_chain_of_fmas_stays_put():
    """The twelve FMAs of a sample (four taps x R, G, B) each leave their sum unchanged, so the bound holds for the whole chain."""
    rng = np.random.default_rng(3)
    for _ in range(500):
        acc = f(rng.uniform(0.5, 4.0) * 2.0 ** int(rng.integers(-90, 90)))
        wgt = f(float(acc * TWO_M25) * rng.uniform(0.0, 1.0))
        a, b = f(rng.uniform(0, 1)), f(rng.uniform(0, 1))
        wa = round_f32(wgt * a); w11 = round_f32(wa * b); w10 = round_f32(wa - w11)
        wt = round_f32(wgt - wa); w01 = round_f32(wt * b); w00 = round_f32(wt - w01)
        for tw in (w00, w10, w01, w11):
            assert 0 <= tw <= wgt                              # monotone roundings keep each tap weight in [0, w]
        q = [f(rng.uniform(0, 1)) for _ in range(4)]       # texels <= M = 1
        r = acc
        for tw, qq in zip((w00, w10, w01, w11), q):
            r = fma_f32(tw, qq, r)
        assert r == acc


def test_subnormal_accumulator_never_qualifies():
    """A subnormal (or zero) sum has no half-ulp margin: the kernel's floor 2^-100 keeps it out; and the lemma would fail there."""
    acc = F(2) ** -140                                        # subnormal
    x = acc * TWO_M25
    assert round_f32(acc + x) == acc                         # (happens to hold here: x is far below the subnormal spacing) ...
    assert round_f32(F(0) + F(2) ** -149) != 0               # ... but a zero sum plainly moves
    assert threshold_f32(0.0, 1.0) == F(2) ** -100 and not (F(0) >= threshold_f32(0.0, 1.0))
    assert not (acc >= threshold_f32(0.0, 1.0))


def threshold_f32(wmax, m):
    """k_mc_region.hip absorb_threshold in exact fp32 steps (left to right, no contraction)."""
    t = round_f32(f(wmax) * f(m))
    t = round_f32(t * (1 + F(1, 2 ** 20)))
    if t > F(float(np.finfo(np.float32).max)):
        return F(10) ** 400                                    # +inf stands in as a huge value
    t = t * 2 ** 25                                          # exact (or overflow, above)
    if t > F(float(np.finfo(np.float32).max)):
        return F(10) ** 400
    return max(t, F(2) ** -100)


def test_fp32_threshold_implies_exact_bound():
    rng = np.random.default_rng(11)
    checked = 0
    for _ in range(4000):
        wmax = float(f32(rng.uniform(0, 1) * 2.0 ** int(rng.integers(-70, 0))))
        m = float(f32(rng.uniform(0, 1) * 2.0 ** int(rng.integers(-60, 40))))
        T = threshold_f32(wmax, m)
        # the smallest sums that pass the test, and some random ones
        for acc in (round_f32(T) if round_f32(T) >= T else next_up(float(round_f32(T))), f(float(T) * rng.uniform(1, 4))):
            if acc >= T and acc < F(10) ** 38:
                assert F(wmax) * F(m) <= acc * TWO_M25, (wmax, m, acc)
                checked += 1
    assert checked > 4000
    # adversarial: W M sitting exactly on acc 2^-25 for acc a power of two, and just above it
    for e in (-100, -50, 0, 50, 100):
        acc = F(2) ** e
        T = threshold_f32(float(2.0 ** (e - 25)), 1.0)
        assert not (acc >= T)                                 # the inflation keeps the exact boundary out (conservative)
        T = threshold_f32(float(2.0 ** (e - 26)), 1.0)
        assert acc >= T
