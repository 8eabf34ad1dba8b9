"""Child process of tests/test_gpu_mc_bin_cache.py: the bin cache's default rule (pbrk_mc_set_bin_cache(-1)) follows the device counters,
and those are read from the environment once per process.  Runs the 64 -> 256^2 (region kernel) and 16 -> 256^2 (resident kernel) levels
with the roughness-0.03 table, registered, once with the cache off and three times under the rule, and prints one JSON line:
{"stats_env": .., "levels": {n_src: {"off": sha, "rule": [sha, sha, sha], "stats": [[recorded, replayed, computed, declined, bytes] x 4]}}}."""
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
    for n_src in (64, 16):
        bord = mc.BorderedLevel(L, level(n_src))
        try:
            L.pbrk_mc_set_bin_cache(0)
            off = hashlib.sha256(mc.filter_windows(L, bord, 0.03, FULL, OUT)).hexdigest()
            L.pbrk_mc_set_bin_cache(-1)
            stats, rule = [list(mc.bin_cache_stats(L).values())], []
            for _ in range(3):
                rule.append(hashlib.sha256(mc.filter_windows(L, bord, 0.03, FULL, OUT)).hexdigest())
                stats.append(list(mc.bin_cache_stats(L).values()))
            res[str(n_src)] = {"off": off, "rule": rule, "stats": stats}
        finally:
            bord.free()
    L.pbrk_mc_table_unregister(dtab.ptr)
    L.GPU_WaitUntilIdle()
    L.GPU_Deinit()
    print(json.dumps({"stats_env": os.environ.get("PBR_MC_STATS"), "levels": res}))


if __name__ == "__main__":
    main()
