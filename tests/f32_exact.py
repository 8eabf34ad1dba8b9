"""Exact fp32 arithmetic for the CPU proofs of the region kernel's skips (test_absorb_lemma_cpu.py, test_mc_launch_cut_cpu.py,
test_mc_launch_cut_slices_cpu.py): round-to-nearest-even on fractions, the same on scaled integers, and bit patterns."""
from fractions import Fraction as F

import numpy as np


def round_f32(q):
    """Exact value q rounded to the nearest fp32, ties to even (no overflow handling: callers stay in range)."""
    if q == 0:
        return F(0)
    sign = -1 if q < 0 else 1
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    while F(2) ** e > a:
        e -= 1
    while F(2) ** (e + 1) <= a:
        e += 1
    e = max(e, -126)                                         # subnormals share the spacing of 2^-126
    ulp = F(2) ** (e - 23)
    k, r = divmod(a, ulp)
    if r > ulp / 2 or (r == ulp / 2 and k % 2 == 1):
        k += 1
    return sign * k * ulp


# The chains of the launch-cut tests run tens of thousands of FMAs.  Every fp32 value is a multiple of 2^-149 and every product of two a multiple of
# 2^-298, so the same exact arithmetic runs on integers scaled by 2^SC (Fraction(x, 2^SC) is the value); test_integer_rounding_is_
# the_fraction_rounding (test_mc_launch_cut_cpu.py) ties the two together.
SC = 400


def to_int(v):
    q = F(float(v)) * 2 ** SC
    assert q.denominator == 1
    return q.numerator


def rnd(x):
    """round_f32 on a non-negative scaled integer"""
    if x == 0:
        return 0
    e = max(x.bit_length() - 1 - SC, -126)
    sh = e - 23 + SC                                          # the ulp as a power of two of the scaled integer
    k, r = x >> sh, x & ((1 << sh) - 1)
    half = 1 << (sh - 1)
    if r > half or (r == half and k & 1):
        k += 1
    return k << sh


def mul(a, b):
    p = a * b
    assert p & ((1 << SC) - 1) == 0
    return p >> SC


def bits(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def from_bits(b):
    return float(np.array([b], dtype=np.uint32).view(np.float32)[0])
