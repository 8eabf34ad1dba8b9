"""What the CPU tests of the launch cut share (test_mc_launch_cut_cpu.py, test_mc_launch_cut_slices_cpu.py): a slice's head sum as
the library adds it, and one sample of the kernel's tap chain in exact fp32 steps on the scaled integers of f32_exact.py."""
from f32_exact import mul, rnd


def head_sum(w, s):
    h = 0.0
    for i in range(32):
        h += float(w[32 * s + i])                             # double, index order
    return h


def tap_weights(wgt, a, b):
    """The kernel's six roundings (tap_accumulate): returns (w00, w10, w01, w11)."""
    wa = rnd(mul(wgt, a)); w11 = rnd(mul(wa, b)); w10 = rnd(wa - w11)
    wt = rnd(wgt - wa); w01 = rnd(mul(wt, b)); w00 = rnd(wt - w01)
    assert 0 <= min(w00, w10, w01, w11) and max(w00, w10, w01, w11) <= wgt
    return w00, w10, w01, w11


def run_sample(acc, wgt, a, b, taps):
    """One sample: four FMAs per sum, in the kernel's order (w00, w10, w01, w11); taps[c] = the four texels of channel c."""
    tw = tap_weights(wgt, a, b)
    out = []
    for c in range(3):
        r = acc[c]
        for k in range(4):
            r = rnd(mul(tw[k], taps[c][k]) + r)
        out.append(r)
    return out
