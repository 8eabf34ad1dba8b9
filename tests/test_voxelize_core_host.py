"""csrc/voxelize_core.h -- the rules the K14 kernels are made of -- compiled for the host and run as a brute-force voxeliser
(tests/voxelize_core_host.cpp: every pixel against every triangle, fragments applied in order) against the numpy reference on the
scenes of the GPU tests: all four fp16 channels of every voxel and the rejected count, bit for bit.  The program is started once per
pass of a scene; that is what this file tests.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "vulkan-pbr-renderer_amd", "python"))
import voxelize_scenes as S  # noqa: E402


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vox_host") / "voxelize_core_host")
    subprocess.run([os.environ.get("CXX", "c++"), "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-I" + os.path.join(ROOT, "vulkan-pbr-renderer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(HERE, "voxelize_core_host.cpp")], check=True)
    return exe


def write_scene(path, scene, ps, grid):
    N = scene["N"]
    ch = S.chains(scene)
    with open(path, "wb") as f:
        sh, sw = scene["sun_map"].shape
        f.write(np.array([N, len(ps["draws"]), sw, sh], np.int32).tobytes())
        f.write(np.ascontiguousarray(scene["sun_map"], np.float32).tobytes())
        f.write(np.ascontiguousarray(grid, np.float16).tobytes())
        for d in ps["draws"]:
            v, ix = scene["meshes"][d["mesh"]]
            v, ix = np.ascontiguousarray(v, np.float32).ravel(), np.ascontiguousarray(ix, np.uint32)
            base, emi = ch[d["material"]]
            bb, eb = (np.concatenate([l.ravel() for l in c]) for c in (base, emi))
            f.write(np.array([len(v), len(ix), d["first_vertex"], d["vertex_count"], d["instance_count"], base[0].shape[1], base[0].shape[0], len(base),
                              emi[0].shape[1], emi[0].shape[0], len(emi), len(bb), len(eb)], np.int32).tobytes())
            f.write(np.concatenate([np.asarray(scene["sun"], np.float32), np.asarray(scene["sun_dir"], np.float32), [np.float32(scene["scale"])]]).astype(np.float32).tobytes())
            f.write(v.tobytes()); f.write(ix.tobytes()); f.write(bb.tobytes()); f.write(eb.tobytes())


def run_host(exe, scene, tmp_path):
    N = scene["N"]
    grid = np.zeros((N, N, N, 4), np.float16) if scene["prior"] is None else scene["prior"]
    grids, rejected = [], 0
    for k, ps in enumerate(scene["passes"]):
        if ps["clear"]:
            grid = np.zeros((N, N, N, 4), np.float16)
        src, dst = str(tmp_path / f"scene{k}.bin"), str(tmp_path / f"grid{k}.bin")
        write_scene(src, scene, ps, grid)
        subprocess.run([exe, src, dst], check=True)
        raw = open(dst, "rb").read()
        rejected += int(np.frombuffer(raw[:8], np.int64)[0])
        grid = np.frombuffer(raw[8:], np.float16).reshape(N, N, N, 4)
        grids.append(grid)
    return grids, rejected


BUILDERS = {"cases": lambda: S.cases_scene(32), "random": S.random_scene, "load": S.load_scene, "two": S.two_pass_scene}


@pytest.mark.parametrize("name", list(BUILDERS))
def test_host_build_of_the_kernel_core_equals_the_reference(host, tmp_path, name):
    scene, want, infos, rej = S.ref_of(name, BUILDERS[name])
    got, hrej = run_host(host, scene, tmp_path)
    assert hrej == rej
    for k, (a, b) in enumerate(zip(got, want)):
        bad = np.argwhere(a.view(np.uint16) != b.view(np.uint16))
        assert len(bad) == 0, (name, k, len(bad), bad[:5].tolist())
