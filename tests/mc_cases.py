"""The shapes the kernel-level tests of the K4b region kernel share (test_gpu_mc_prologue.py, _launch_cut.py, _tile32.py and the
CPU twin test_mc_launch_cut_cpu.py): row windows of 256^2 levels, the smallest the region kernel accepts.  Nothing of the GPU side
is imported here."""
import numpy as np

OUT = 256
# (face0, face1, y0, rows): the tangent frame's pole rows 63 and 192 on faces +-X; a ragged window on the others
WINDOWS = [(0, 2, 48, 32), (0, 2, 176, 32), (2, 6, 53, 37)]
FULL = [(0, 6, 0, OUT)]


def level(n_src, seed=7):
    return np.random.default_rng(seed + n_src).random((6, n_src, n_src, 4), dtype=np.float32) + 0.1
