"""K17 without a GPU: the numpy restatement (tests/sh_ref.py) against closed forms, band-limited inputs and the reference's
irradiance shader arithmetic (the CPU oracle); csrc/sh_core.h compiled for the host (tests/sh_core_host.cpp), plain and with
ASan + UBSan, against the restatement; the host functions of pbr_sh.c (file round trip, evaluation)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import sh_ref as R  # noqa: E402

CSRC = os.path.join(ROOT, "vulkan-pbr-renderer_amd", "csrc")
PROJECT_TOL = 1e-10                     # x S[k][c]; derivation in tests/test_gpu_sh.py
SYNTH_TOL = 2.0 ** -22                  # x sum_k |a_k coef Y_k|: one fp32 rounding (2^-24) with fourfold margin


# ---- the restatement against closed forms ----
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 16, 64, 256])
def test_solid_angles_sum_to_the_sphere(n):
    w = R.solid_angles(n)
    err = abs(6.0 * w.sum() - 4.0 * np.pi)
    print(f"n={n}: |6 sum domega - 4 pi| = {err:.3g} / tolerance 1e-13")
    assert w.shape == (n, n) and (w > 0).all() and err <= 1e-13
    assert np.array_equal(w, w.T) and np.allclose(w, w[::-1, ::-1], rtol=0, atol=1e-15)      # the face's symmetry


def test_constant_cube():
    for n, c in ((1, 1.0), (5, 0.25), (16, 1000.0)):
        cube = np.full((6, n, n, 4), c, np.float32)
        coef, S = R.project(cube)
        assert np.abs(coef[0] - c * np.sqrt(4.0 * np.pi)).max() <= 1e-12 * c
        assert np.abs(coef[1:]).max() <= 1e-12 * c, np.abs(coef[1:]).max()
        assert np.abs(R.irradiance(coef, 4) - c / 2.0).max() <= 1e-12 * c
        assert (S >= np.abs(coef)).all()


def test_directions_are_unit_and_match_the_face_table():
    d = R.directions(4)
    assert np.abs(np.linalg.norm(d, axis=-1) - 1.0).max() < 1e-15
    for f, axis, sign in ((0, 0, 1), (1, 0, -1), (2, 1, 1), (3, 1, -1), (4, 2, 1), (5, 2, -1)):
        assert (sign * d[f, ..., axis] > 0.5).all()
    assert d[0, 0, 0, 1] > 0 and d[0, 0, 0, 2] > 0 and d[4, 0, 3, 0] > 0 and d[2, 3, 0, 2] > 0      # (1, -tc, -sc), (sc, -tc, 1), (sc, 1, tc)


def test_band_limited_recovery():
    c = np.random.default_rng(1).standard_normal((9, 3))
    err = {}
    for n in (64, 256):
        got, _ = R.project(R.band_limited_cube(n, c))
        err[n] = np.abs(got - c).max()
    print(f"band-limited recovery: n=64 {err[64]:.3g} / 1e-3; n=256 {err[256]:.3g} / {err[64] / 8:.3g}")
    assert err[64] <= 1e-3 and err[256] <= err[64] / 8.0


def test_normalisation_and_axes_against_the_reference_shader_arithmetic():
    """gen_irradiance_map.glsl on the CPU oracle, 1024 samples of LOD 0 of a band-limited cube: the residue is that quadrature;
    a wrong factor or a swapped axis gives O(1)."""
    import pbr_oracle as O
    c = np.random.default_rng(2).standard_normal((9, 3))
    c[0] = 6.0
    cube = R.band_limited_cube(64, c)
    want = O.irradiance(O.build_pyramid(cube), 64, out_size=8, src_lod=0, nsamples=1024)[..., :3].astype(np.float64)
    got = R.irradiance(R.project(cube)[0], 8)
    err = np.abs(got - want).max()
    print(f"SH9 irradiance vs shader arithmetic: max abs {err:.3g} / 5e-3 at mean {want.mean():.3g}")
    assert 0.5 < want.mean() < 1.5 and err <= 5e-3


# ---- the host build of sh_core.h ----
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sh_host") / ("sh_core_host_" + request.param))
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if request.param == "sanitized" else []
    subprocess.run([os.environ.get("CXX", "c++"), "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-I" + CSRC, "-o", exe,
                    os.path.join(HERE, "sh_core_host.cpp")], check=True)
    return exe


def run_host(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stdout[-500:], r.stderr[-3000:])


PROJECT_CASES = [(1, (0, 6), None), (3, (0, 6), None), (5, (0, 6), None), (64, (0, 6), None), (96, (0, 6), None), (64, (1, 4), (7, 29))]


def test_host_projection_equals_the_restatement(host, tmp_path):
    for n, faces, rows in PROJECT_CASES:
        cube = R.hdr_cube(n, 100 + n)
        src, dst = str(tmp_path / "level.bin"), str(tmp_path / "coef.bin")
        cube.tofile(src)
        r0, r1 = rows or (0, n)
        run_host(host, "project", n, faces[0], faces[1], r0, r1, src, dst)
        got = np.fromfile(dst, np.float64).reshape(9, 3)
        want, S = R.project(cube, faces, rows)
        worst = R.worst_ratio(np.abs(got - want), S)
        print(f"host projection n={n} faces={faces} rows={rows}: worst {worst:.3g} / tolerance {PROJECT_TOL:g} of S")
        assert worst <= PROJECT_TOL


def test_host_solid_angles_equal_the_restatement(host, tmp_path):
    for n in (1, 5, 64):
        dst = str(tmp_path / "omega.bin")
        run_host(host, "omega", n, dst)
        got, want = np.fromfile(dst, np.float64).reshape(n, n), R.solid_angles(n)
        # four atan2 of magnitude <= 0.62, a few ulp each (the derivation in tests/test_gpu_sh.py)
        assert np.abs(got - want).max() <= 16 * 2.0 ** -53 * 0.62


def test_host_synthesis_equals_the_restatement(host, tmp_path):
    coef, _ = R.project(R.hdr_cube(16, 7))
    src, dst = str(tmp_path / "coef.bin"), str(tmp_path / "irr.bin")
    coef.tofile(src)
    for size in (1, 3, 32, 40):
        run_host(host, "irradiance", size, src, dst)
        got = np.fromfile(dst, np.float32).reshape(6, size, size, 4)
        want, bound = R.irradiance(coef, size), R.irradiance_bound(coef, size)
        worst = R.worst_ratio(np.abs(got[..., :3] - want), bound)
        print(f"host synthesis size={size}: worst {worst:.3g} / tolerance {SYNTH_TOL:.3g} of sum |a c Y|")
        assert worst <= SYNTH_TOL and not got[..., 3].view(np.uint32).any()


def test_host_program_refuses_bad_arguments(host, tmp_path):
    short = str(tmp_path / "short.bin")
    np.zeros(10, np.float32).tofile(short)
    for args in (["project", 4, 0, 6, 0, 4, short, short], ["project", 4, 0, 7, 0, 4, short, short], ["project", 4, 0, 6, 3, 3, short, short],
                 ["irradiance", 0, short, short], ["omega", -1, short], ["nothing"]):
        r = subprocess.run([host, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode in (2, 3), (args, r.returncode, r.stderr[-2000:])


# ---- the host functions of pbr_sh.c (no GPU call) ----
@pytest.fixture(scope="module")
def L():
    import pbrhip
    if not os.path.exists(pbrhip.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(pbrhip.PKG_ROOT, "csrc"), "-j", "8"], stdout=subprocess.DEVNULL)
    return pbrhip.lib()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_sh9_file_round_trip_keeps_every_bit(L, tmp_path):
    rng = np.random.default_rng(3)
    coef = rng.standard_normal(27) * 10.0 ** rng.integers(-12, 12, 27)
    coef[5], coef[6], coef[7] = 0.0, -0.0, 5e-324
    path = str(tmp_path / "env.sh9").encode()
    assert L.PBR_WriteSH9File(path, _dp(coef)) == 0
    back = np.full(27, np.nan)
    assert L.PBR_ReadSH9File(path, _dp(back)) == 0
    assert back.tobytes() == coef.tobytes()
    lines = open(path).read().split("\n")
    assert lines[0].startswith("#") and "Condon" in lines[0] and len(lines) == 11 and lines[10] == ""
    assert all(len(l.split()) == 3 for l in lines[1:10])


def test_sh9_file_reader_refuses_truncated_and_garbled_files(L, tmp_path):
    coef = np.arange(27, dtype=np.float64) + 0.5
    good = str(tmp_path / "good.sh9")
    assert L.PBR_WriteSH9File(good.encode(), _dp(coef)) == 0
    text = open(good).read()
    lines = text.split("\n")
    bad = {
        "truncated_line": "\n".join(lines[:9]) + "\n",
        "truncated_mid": text[:len(text) - 8],
        "no_header": "\n".join(lines[1:]),
        "garbled": text.replace("4.5", "4.x"),
        "two_values": "\n".join(lines[:3] + [lines[3].rsplit(" ", 1)[0]] + lines[4:]),
        "four_values": "\n".join(lines[:3] + [lines[3] + " 1"] + lines[4:]),
        "trailing": text + "1 2 3\n",
        "empty": "",
    }
    for name, content in bad.items():
        p = str(tmp_path / (name + ".sh9"))
        with open(p, "w") as f:
            f.write(content)
        out = np.full(27, -7.0)
        assert L.PBR_ReadSH9File(p.encode(), _dp(out)) != 0, name
        assert (out == -7.0).all(), name                                       # a refused file writes nothing
    assert L.PBR_ReadSH9File(str(tmp_path / "missing.sh9").encode(), _dp(np.zeros(27))) != 0
    assert L.PBR_WriteSH9File(str(tmp_path / "no_such_dir" / "x.sh9").encode(), _dp(coef)) != 0


def test_eval_equals_the_restatement(L):
    rng = np.random.default_rng(4)
    coef, _ = R.project(R.hdr_cube(16, 7))
    flat = np.ascontiguousarray(coef.reshape(27))
    dirs = rng.standard_normal((64, 3)).astype(np.float32)
    dirs[0] = (0, 0, 2)                                                        # not unit: the function normalises
    worst = 0.0
    for n in dirs:
        rgb = np.zeros(3, np.float32)
        L.PBR_EvalSH9Irradiance(_dp(flat), n.ctypes.data_as(C.POINTER(C.c_float)), rgb.ctypes.data_as(C.POINTER(C.c_float)))
        d = n.astype(np.float64) / np.linalg.norm(n.astype(np.float64))
        want, bound = R.irradiance(coef, d), R.irradiance_bound(coef, d)
        worst = max(worst, R.worst_ratio(np.abs(rgb - want), bound))
    print(f"PBR_EvalSH9Irradiance: worst {worst:.3g} / tolerance {SYNTH_TOL:.3g} of sum |a c Y|")
    assert worst <= SYNTH_TOL
