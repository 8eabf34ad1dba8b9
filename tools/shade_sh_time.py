#!/usr/bin/env python3
"""K5.shade with the ambient term from the irradiance cube against the same pass in SH9 mode (PBR_LightingUseSH9), timed on the GPU:
  c3        1920x1080 metal-rough-spheres G-buffer (bench.py's C3), whole frame, RGBA16F target
  c5_band   rows [2160, 3240) of the 7680x4320 'temple' G-buffer (bench.py's C5: the third of four screen bands, ground and columns)
Per-op HIP-event times (GPUX_GraphTimedOpMs) of `--ops` draws back to back in one graph on one stream, GPUX_SetLevelOverlap(0); one
repetition is one such submission and its figure the mean over its ops.  Cube path and SH path alternate, `--reps` repetitions each;
min and spread (max - min) over the repetitions are reported.  With --parent-lib the cube path is measured the same way with that
library (the parent commit's libgpu_hip.so) in a process of its own, before and after this tree's, in the same session.
The c3 case also reports, as numbers, the largest difference between the SH frame and the cube-path frame whose irradiance cube is
K17's synthesis of the same coefficients at 32^2 and at 128^2 (RGBA32F targets): the bilinear error of the cube that SH mode removes.
Every case runs in a child process of its own under `timeout`; the first failure ends the run.  Needs the GPU; there is no fallback.
    python3 tools/shade_sh_time.py [--parent-lib PATH] [--out profiles/shade_sh9.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vulkan-pbr-renderer_amd", "python"))

CASES = ("c3", "c5_band")
LIMIT_S = {"c3": 240, "c5_band": 420}
NEW_SYMBOLS = ("GPUX_GetShadeFlags", "GPUX_SetShadeSH9", "PBR_LightingUseSH9")


def run_case(case, ops, reps, lib_path):
    import numpy as np
    import pbrhip
    from pbrhip import synth
    parent = lib_path is not None
    if parent:
        pbrhip.LIB_PATH = lib_path
        for n in NEW_SYMBOLS:
            pbrhip.PROTOTYPES.pop(n, None)
    if case == "c3":
        W, H, rows = 1920, 1080, (0, 0)
        gbd = synth.synth_gbuffer_spheres(W, H)
    else:
        W, H, rows = 7680, 4320, (2160, 3240)
        gbd = synth.synth_gbuffer_temple(W, H, rows=rows, workers=min(16, os.cpu_count() or 1))      # forked workers: before the GPU is touched
    L = pbrhip.init(0)
    L.GPUX_SetLevelOverlap(0)
    env = synth.synth_env(256, seed=0x5EED0003)
    env_tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 256, 256, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), 32, 256, 256)                           # render.cpp:794-796
    L.PBR_GenIrradianceMap(env_tex, maps.irradiance_map)
    L.PBR_GenPrefilteredEnvMap(env_tex, maps.tex_specular_env_map, 16)
    L.PBR_GenBRDFIntegrationMap(maps.brdf_lut)
    glob = pbrhip.fill_globals(gbd["cam_pos"], aspect=W / H)

    def gbuffer(fmt):
        gb = pbrhip.PBR_GBuffer()
        L.PBR_MakeGBuffer(C.byref(gb), W, H, fmt)
        for name, key in (("base_color", "base"), ("normal", "normal"), ("orm", "orm"), ("emissive", "emissive"), ("depth", "depth")):
            pbrhip.upload_mip(getattr(gb, name), 0, gbd[key])
        return gb

    gb = gbuffer(pbrhip.Format_RGBA16F)
    lp = L.PBR_MakeLightingPass(C.byref(gb), C.byref(maps), W, H)
    g = L.GPU_MakeGraph()
    coef_buf = None
    if not parent:
        coef_buf = L.GPU_MakeBuffer(216, pbrhip.BufferFlag_GPU, None)
        L.GPUX_OpProjectSH9(g, env_tex, 0, 0, 6, 0, 256, coef_buf, 0)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    L.GPUX_EnableOpTiming(1)

    def rep(sh):
        if not parent:
            L.PBR_LightingUseSH9(lp, coef_buf if sh else None, 0)
        for _ in range(ops):
            L.PBR_RecordLightingPass(lp, g, C.byref(glob), rows[0], rows[1])
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        us = [L.GPUX_GraphTimedOpMs(g, i) * 1e3 for i in range(L.GPUX_GraphTimedOpCount(g)) if L.GPUX_GraphTimedOpName(g, i) == b"K5.shade"]
        assert len(us) == ops, len(us)
        return float(np.mean(us)), float(np.min(us))

    modes = ("cube",) if parent else ("cube", "sh9")
    for m in modes:                                                           # warm-up: twins, clocks
        rep(m == "sh9")
    times = {m: [] for m in modes}
    for _ in range(reps):
        for m in modes:
            times[m].append(rep(m == "sh9"))
    res = {"case": case, "library": "parent" if parent else "this tree", "width": W, "height": H, "rows": rows if rows[1] else (0, H),
           "ops_per_repetition": ops, "repetitions": reps}
    for m in modes:
        means = [t[0] for t in times[m]]
        res[m] = {"min_us": min(means), "max_us": max(means), "spread_us": max(means) - min(means), "fastest_op_us": min(t[1] for t in times[m]),
                  "repetition_means_us": means}
    if not parent:
        res["sh9_over_cube_min"] = res["sh9"]["min_us"] / res["cube"]["min_us"]
    L.GPUX_EnableOpTiming(0)

    if case == "c3" and not parent:                                          # the bilinear error of the cube that SH mode removes
        gb32 = gbuffer(pbrhip.Format_RGBA32F)
        coef = pbrhip.project_sh9(env_tex, 0)

        def frame(lighting_pass):
            L.PBR_RecordLightingPass(lighting_pass, g, C.byref(glob), 0, 0)
            L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
            return pbrhip.read_mip(gb32.lighting_result, 0)[..., :3].astype(np.float64)

        lp_sh = L.PBR_MakeLightingPass(C.byref(gb32), C.byref(maps), W, H)
        L.PBR_LightingUseSH9(lp_sh, coef_buf, 0)
        sh_frame = frame(lp_sh)
        res["sh9_frame_vs_cube_of_the_same_coefficients"] = []
        for size in (32, 128):
            cube = pbrhip.make_texture(pbrhip.Format_RGBA32F, size, size, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_StorageImage, None)
            pbrhip.irradiance_from_sh9(coef, cube, 0)
            m2 = pbrhip.PBR_IBLMaps()
            m2.irradiance_map, m2.brdf_lut, m2.tex_specular_env_map = cube, maps.brdf_lut, maps.tex_specular_env_map
            lp2 = L.PBR_MakeLightingPass(C.byref(gb32), C.byref(m2), W, H)
            cube_frame = frame(lp2)
            diff = np.abs(sh_frame - cube_frame)
            res["sh9_frame_vs_cube_of_the_same_coefficients"].append(
                {"cube_size": size, "max_abs": float(diff.max()), "max_rel_floor_1e-2": float((diff / np.maximum(np.abs(cube_frame), 1e-2)).max())})
            L.PBR_DestroyLightingPass(lp2); L.GPU_DestroyTexture(cube)
        L.PBR_DestroyLightingPass(lp_sh)
        L.PBR_DestroyGBuffer(C.byref(gb32))
    L.GPU_WaitUntilIdle()
    L.GPU_Deinit()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_sh9.json"))
    ap.add_argument("--ops", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libgpu_hip.so of the parent commit: its cube path is measured in the same session")
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON line")
    ap.add_argument("--lib", default=None, help="with --case: the library to load instead of this tree's")
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.ops, args.reps, args.lib)))
        return 0
    assert args.reps >= 5
    out = {"what": "K5.shade per-op HIP-event time (GPUX_GraphTimedOpMs), draws back to back in one graph; cube path and SH9 path alternate; "
                   "one repetition = the mean over the draws of one submission; min and spread over the repetitions", "runs": []}
    for case in CASES:
        legs = [None] if not args.parent_lib else [args.parent_lib, None, args.parent_lib]
        for lib in legs:
            cmd = ["timeout", "-k", "10", str(LIMIT_S[case]), sys.executable, os.path.abspath(__file__), "--case", case, "--ops", str(args.ops),
                   "--reps", str(args.reps)] + (["--lib", os.path.abspath(lib)] if lib else [])
            r = subprocess.run(cmd, capture_output=True, text=True)
            lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not lines:
                print(f"{case} ({lib or 'this tree'}): exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
                return 1                                                      # nothing more is started on the GPU
            res = json.loads(lines[-1][len("RESULT "):])
            out["runs"].append(res)
            for m in ("cube", "sh9"):
                if m in res:
                    print(f"{case} {res['library']} {m}: min {res[m]['min_us']:.1f} us, spread {res[m]['spread_us']:.1f} us, fastest op {res[m]['fastest_op_us']:.1f} us", flush=True)
            for d in res.get("sh9_frame_vs_cube_of_the_same_coefficients", ()):
                print(f"    SH frame vs {d['cube_size']}^2 cube of the same coefficients: max abs {d['max_abs']:.3e}, max rel {d['max_rel_floor_1e-2']:.3e}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
