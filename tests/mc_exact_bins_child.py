"""Child process of tests/test_gpu_mc_exact_bins.py: the default rule of pbrk_mc_set_exact_bins(-1) follows the device counters, which are
read from the environment once per process, and takes the kernel shapes measured as a gain (the 34^2 shape: n_src 32; the 66^2
whole-face shape, n_src 64, is left out by the host rule).  The bin cache is asked for by name (on), the refinement is left to its rule.
Runs the 64 -> 256^2 and 32 -> 256^2 levels with the roughness-0.03 table, registered, once with the cache off and three times with it on, and
prints one JSON line: {"stats_env": .., "levels": {n_src: {"off": sha, "on": [sha x 3], "last_exact": 0 | 1, "moved": [recorded,
replayed]}}, "exact": pbrk_mc_exact_bins_stats by name}."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(os.path.dirname(HERE), "vulkan-pbr-renderer_amd", "python")):
    sys.path.insert(0, p)

import pbrhip                                                      # noqa: E402
from mc_cases import FULL, OUT, level                              # noqa: E402
from pbrhip import mc                                              # noqa: E402


def main():
    L = pbrhip.init()
    dtab, n_full, _ = mc.prefilter_table(L, 0.03)
    assert L.pbrk_mc_table_register(dtab.ptr, n_full) == 0
    res = {}
    for n_src in (64, 32):
        bord = mc.BorderedLevel(L, level(n_src))
        try:
            L.pbrk_mc_set_bin_cache(0)
            off = hashlib.sha256(mc.filter_windows(L, bord, 0.03, FULL, OUT)).hexdigest()
            L.pbrk_mc_set_bin_cache(1)
            before = mc.bin_cache_stats(L)
            on = [hashlib.sha256(mc.filter_windows(L, bord, 0.03, FULL, OUT)).hexdigest()]
            last = L.pbrk_mc_last_exact_bins()
            on += [hashlib.sha256(mc.filter_windows(L, bord, 0.03, FULL, OUT)).hexdigest() for _ in range(2)]
            after = mc.bin_cache_stats(L)
            res[str(n_src)] = {"off": off, "on": on, "last_exact": last,
                               "moved": [after["recorded"] - before["recorded"], after["replayed"] - before["replayed"]]}
        finally:
            bord.free()
    exact = mc.exact_bins_stats(L)
    L.pbrk_mc_table_unregister(dtab.ptr)
    L.GPU_WaitUntilIdle()
    L.GPU_Deinit()
    print(json.dumps({"stats_env": os.environ.get("PBR_MC_STATS"), "levels": res, "exact": exact}))


if __name__ == "__main__":
    main()
