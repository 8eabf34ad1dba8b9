#!/usr/bin/env python3
"""K17 (SH9 projection and irradiance) timed on the GPU, next to the project's two HBM-shaped yardsticks in the same session:
  project_4096 / project_1024 / project_256   HIP-event time of K17.sh_project (both launches: partials + their sum) over a whole
                                               level, `--ops` ops back to back in one graph (GPUX_GraphTimedOpMs), median
  split_4096                                   the same op on parts of a 4096^2 level -- faces [0, 6), [0, 2), [0, 1) of all rows, all faces
                                               of half the rows and of 64 rows: what a row costs whatever the faces, and one wave's pace
  irradiance_128                               K17.sh_irradiance into a 128^2 cube, the same way
  k4a_copy_4096                                K4a.prefilter_copy.mip0 of a 4096^2 specular cube from a 2048^2 environment (README: 0.80)
  k2_mip_chain_2048                            K2.mip_chain of a 2048^2 environment (README: 0.56-0.66)
Bytes are the algorithm's (16 B read per texel of the projected level; 16 B written per texel synthesised; K4a: target written +
source level read once; K2: every level read once, every level but the first written once) and are reported over the median time as
a fraction of 8 TB/s.  Every case runs in a child process of its own under `timeout`; the first failure ends the run.
Needs the GPU; there is no fallback.
    python3 tools/sh_time.py [--out profiles/sh_project.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vulkan-pbr-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ("project_4096", "project_1024", "project_256", "split_4096", "irradiance_128", "k4a_copy_4096", "k2_mip_chain_2048")
LIMIT_S = {"project_4096": 240, "split_4096": 240}                                               # 1.6 GB of host noise + upload; the others: 120


def timed_ops(L, g, name):
    return [L.GPUX_GraphTimedOpMs(g, i) * 1e3 for i in range(L.GPUX_GraphTimedOpCount(g)) if L.GPUX_GraphTimedOpName(g, i).startswith(name)]


def run_case(case, ops):
    import numpy as np
    import pbrhip
    L = pbrhip.init(0)
    rng = np.random.default_rng(17)
    kind, n = case.rsplit("_", 1)
    n = int(n)
    g = L.GPU_MakeGraph()
    res = {"case": case, "ops": ops}

    def measure(record, name):
        us = []
        for _ in range(2):                                                    # submission 0 warms up
            for _ in range(ops):
                record()
            L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
            us = timed_ops(L, g, name)
        assert len(us) == ops, (name, len(us))
        return sorted(us)

    def noise_cube(size, flags):
        data = (rng.random((6, size, size, 4), dtype=np.float32) ** 8) * np.float32(1000.0)
        return pbrhip.make_texture(pbrhip.Format_RGBA32F, size, size, pbrhip.TextureFlag_Cubemap | flags, data), data

    if kind == "project":
        tex, data = noise_cube(n, 0)
        buf = L.GPU_MakeBuffer(216, pbrhip.BufferFlag_GPU, None)
        first = pbrhip.project_sh9(tex, 0)
        assert first.tobytes() == pbrhip.project_sh9(tex, 0).tobytes()        # deterministic
        if n <= 256:
            import sh_ref
            want, S = sh_ref.project(data)
            res["worst_error_over_S"] = sh_ref.worst_ratio(np.abs(first - want), S)
            assert res["worst_error_over_S"] <= 1e-10
        res["coef_L00"] = first[0].tolist()
        L.GPUX_EnableOpTiming(1)
        us = measure(lambda: L.GPUX_OpProjectSH9(g, tex, 0, 0, 6, 0, n, buf, 0), b"K17.sh_project")
        res["bytes"] = 6 * n * n * 16
        res["scratch_bytes"] = int(L.pbrk_sh9_scratch_bytes(n))
    elif kind == "split":
        tex, _ = noise_cube(n, 0)
        buf = L.GPU_MakeBuffer(216, pbrhip.BufferFlag_GPU, None)
        L.GPUX_EnableOpTiming(1)
        res["parts"] = []
        for faces, rows in (((0, 6), (0, n)), ((0, 2), (0, n)), ((0, 1), (0, n)), ((0, 6), (0, n // 2)), ((0, 6), (0, 64))):
            us = measure(lambda: L.GPUX_OpProjectSH9(g, tex, 0, faces[0], faces[1], rows[0], rows[1], buf, 0), b"K17.sh_project")
            res["parts"].append({"faces": faces, "rows": rows, "median_us": us[len(us) // 2]})
        us = [p["median_us"] for p in res["parts"][:1]]
        res["bytes"] = 6 * n * n * 16
    elif kind == "irradiance":
        tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, n, n, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_StorageImage, None)
        coef = rng.standard_normal(27)
        buf = L.GPU_MakeBuffer(216, pbrhip.BufferFlag_GPU, coef.ctypes.data_as(C.c_void_p))
        L.GPUX_EnableOpTiming(1)
        us = measure(lambda: L.GPUX_OpIrradianceFromSH9(g, buf, 0, tex, 0), b"K17.sh_irradiance")
        res["bytes"] = 6 * n * n * 16
    elif kind == "k4a_copy":
        env, _ = noise_cube(n // 2, pbrhip.TextureFlag_HasMipmaps)
        maps = pbrhip.PBR_IBLMaps()
        L.PBR_MakeIBLMaps(C.byref(maps), 8, 64, n)
        pipes, arena = L.PBR_MakeIBLPipelines(), L.GPU_MakeDescriptorArena()
        arr = (pbrhip.PBR_WorkUnit * 1)(pbrhip.PBR_WorkUnit(pbrhip.Unit_Prefilter, 0, 0, 6, 0, n, 0.0))
        L.GPUX_EnableOpTiming(1)
        us = measure(lambda: L.PBR_RecordUnits(pipes, g, arena, env, C.byref(maps), arr, 1), b"K4a.prefilter_copy")
        res["bytes"] = 6 * n * n * 16 + 6 * (n // 4) ** 2 * 16                # target written + source LOD 1 read once
    elif kind == "k2_mip_chain":
        env, _ = noise_cube(n, pbrhip.TextureFlag_HasMipmaps)
        L.GPUX_EnableOpTiming(1)
        us = measure(lambda: L.GPU_OpGenerateMipmaps(g, env), b"K2.mip_chain")
        levels = [max(1, n >> m) for m in range(env.contents.mip_level_count)]
        res["bytes"] = sum(6 * s * s * 16 for s in levels[:-1]) + sum(6 * s * s * 16 for s in levels[1:])
    else:
        raise SystemExit(f"unknown case {case}")
    L.GPUX_EnableOpTiming(0)
    med = us[len(us) // 2]
    res.update(median_us=med, min_us=us[0], max_us=us[-1], fraction_of_8TBps=res["bytes"] / (med * 1e-6) / 8e12)
    L.GPU_WaitUntilIdle()
    L.GPU_Deinit()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sh_project.json"))
    ap.add_argument("--ops", type=int, default=20)
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON line")
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.ops)))
        return 0
    out = {"what": "K17 SH9 projection / irradiance, per-op HIP-event time (GPUX_GraphTimedOpMs), ops back to back in one graph; "
                   "K4a and K2 measured the same way in the same session", "cases": []}
    for case in CASES:
        limit = LIMIT_S.get(case, 120)
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", case, "--ops", str(args.ops)],
                           capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(f"{case}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 1                                                          # nothing more is started on the GPU
        res = json.loads(lines[-1][len("RESULT "):])
        out["cases"].append(res)
        print(f"{case}: median {res['median_us']:.1f} us ({res['min_us']:.1f} .. {res['max_us']:.1f}), {res['bytes'] / 1e6:.1f} MB = "
              f"{res['fraction_of_8TBps']:.3f} of 8 TB/s", flush=True)
        for part in res.get("parts", ()):
            print(f"    faces {part['faces']} rows {part['rows']}: median {part['median_us']:.1f} us", flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
