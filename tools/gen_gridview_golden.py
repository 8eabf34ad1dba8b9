#!/usr/bin/env python3
"""tests/golden/gridview_shader_text.npz: the light-grid visualiser (lighting_pass.glsl:463-491, Globals.visualize_lightgrid = 1) as the
REFERENCE's shader text computes it, on views A and B of tests/gridview_ref.py (pbrhip.synth.synth_gi_scene(96, 54), 128^3 grid).

Runs only where the reference tree exists.  It imports the unchanged oracle/gen_oracle_a.py and builds `lighting_full` exactly as its
gen_gi does (DRIVER_LIGHTING_FULL, variant live_shaft, -DSHIM_DET_TRIG -DSHIM_SAMPLER_IDS: the shader text compiled against
oracle/glsl_shim.hpp, LIGHTGRID sampled by the oracle's orc_tex3d_sample); the Globals come from ref_fill_globals of
oracle/_ref/libref_thirdparty.so (the reference's own camera / matrix code).  The fixture is data only: two fp32 [54][96][4] frames and
the two 138-word Globals (word 137 = 1).  This file holds no reference text."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_oracle_a as A  # noqa: E402
import gridview_ref as V  # noqa: E402


def main():
    from pbrhip import synth
    W, H = V.W, V.H
    gbd, grid, levels, sun = synth.synth_gi_scene(W, H)
    subprocess.check_call(["make", "-C", A.HERE, "ref"], stdout=subprocess.DEVNULL)
    R = C.CDLL(os.path.join(A.HERE, "_ref", "libref_thirdparty.so"))
    os.makedirs(A.SCRATCH, exist_ok=True)
    S = A.SCRATCH
    gb = os.path.join(S, "gv_gbuffer.bin")
    with open(gb, "wb") as f:
        for k in ("base", "normal", "orm", "emissive"):
            f.write(np.ascontiguousarray(gbd[k]).tobytes())
        f.write(np.ascontiguousarray(gbd["depth"], np.float32).tobytes())
    grp = os.path.join(S, "gv_grid.bin"); np.ascontiguousarray(grid).tofile(grp)
    pp = os.path.join(S, "gv_prev.bin")
    with open(pp, "wb") as f:
        for lv in levels:
            f.write(np.ascontiguousarray(lv).tobytes())
    sp = os.path.join(S, "gv_sun.bin"); sun.tofile(sp)
    A.CXX.extend(["-DSHIM_DET_TRIG", "-DSHIM_SAMPLER_IDS"])
    try:
        exe = A.build("lighting_full", "lighting_pass.glsl", A.DRIVER_LIGHTING_FULL, lighting_variant="live_shaft")
    finally:
        del A.CXX[-2:]
    out = {}
    for view, ori, default_ori in (("A", (0, 0, 0, 1), 1), ("B", V.ORI_B, 0)):
        gbuf = np.zeros(140, np.float32)
        R.ref_fill_globals((C.c_float * 3)(*synth.GI_SCENE_CAMERA), (C.c_float * 4)(*ori), default_ori, C.c_float(75), C.c_float(W / H),
                           C.c_float(.02), C.c_float(1e4), C.c_float(56.5), C.c_float(97), V.FRAME_IDX, gbuf.ctypes.data_as(C.c_void_p))
        gbuf[136] = 1.0 / synth.GI_SCENE_EXTENT
        gbuf.view(np.uint32)[137] = 1
        gp = os.path.join(S, "gv_globals.bin"); gbuf.tofile(gp)
        outp = os.path.join(S, "gv_out.bin")
        subprocess.check_call([exe, str(W), str(H), gp, gb, grp, str(grid.shape[0]), pp, str(levels[0].shape[1]), str(levels[0].shape[0]),
                               str(len(levels)), sp, str(sun.shape[1]), str(sun.shape[0]), outp])
        out["frame_" + view] = np.fromfile(outp, dtype=np.float32).reshape(H, W, 4)
        out["globals_" + view] = gbuf[:138].copy()
        lit = (out["frame_" + view][..., :3] > 0).any(-1)
        print("view", view, ": pixels with a hit colour", int(lit.sum()), "of", W * H)
    if out["globals_A"][:137].tobytes() != np.load(os.path.join(A.GOLDEN, "ref_globals_gi_scene.npy"))[:137].tobytes():
        raise SystemExit("view A's Globals differ from tests/golden/ref_globals_gi_scene.npy")
    np.savez_compressed(V.FIXTURE, **out)
    print("wrote", V.FIXTURE, os.path.getsize(V.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
