"""csrc/bc6h2_core.h -- the two-region quality level of the K18 encode contract -- compiled for the host (tests/bc6h_encode_host.cpp at
quality 1), plain and with ASan + UBSan, against the numpy restatement (tests/bc6h2_ref.py), byte for byte; the restatement's blocks through the
independent decoder of tests/bc6h_decode_ref.py (pinned to Pillow by the K19 tests), which proves the packing; and the properties of
the contract.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bc6h2_ref as R2  # noqa: E402
import bc6h_decode_ref as D  # noqa: E402
import bc6h_host_build  # noqa: E402
import bc6h_ref as R  # noqa: E402
from bc6h_host_build import CSRC  # noqa: E402


@pytest.fixture(scope="module", params=bc6h_host_build.VARIANTS)
def host(request, tmp_path_factory):
    return bc6h_host_build.build("bc6h_encode_host.cpp", request.param, tmp_path_factory)


@pytest.fixture(scope="module")
def encoded():
    """name -> (level, half codes per block, blocks of the contract, what the search chose): computed once, never written to"""
    out = {}
    for name, lvl in R2.cases():
        h = R.block_texels(R.half_codes(lvl))
        blocks, chosen = R2.encode2_blocks(h)
        for a in (h, blocks, *chosen.values()):
            a.setflags(write=False)
        out[name] = (lvl, h, blocks, chosen)
    return out


def run_host(exe, tmp_path, level):
    layers, h, w, _ = level.shape
    src, dst, info = str(tmp_path / "texels.bin"), str(tmp_path / "blocks.bin"), str(tmp_path / "info.bin")
    level.tofile(src)
    r = subprocess.run([exe, "1", "0" if level.dtype == np.float32 else "1", str(w), str(h), str(layers), src, dst, info], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    return np.fromfile(dst, np.uint8).reshape(-1, 16), np.fromfile(info, np.uint64).reshape(-1, 3).astype(np.int64)


def test_bc6h2_core_header_exists():
    assert os.path.isfile(os.path.join(CSRC, "bc6h2_core.h")) and os.path.isfile(os.path.join(CSRC, "bc6h_format.h"))


def test_host_build_of_the_two_region_core_equals_the_restatement(host, tmp_path, encoded):
    """blocks byte for byte, and the kind, partition and error the header reports per block"""
    for name, (lvl, _, want, chosen) in encoded.items():
        got, info = run_host(host, tmp_path, lvl)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        bad = np.argwhere((got != want).any(axis=1)).ravel()
        assert len(bad) == 0, (name, len(bad), bad[:5].tolist(), got[bad[:1]].tolist(), want[bad[:1]].tolist())
        assert np.array_equal(info[:, 0], chosen["kind"]) and np.array_equal(info[:, 2], chosen["err"]), name
        two = chosen["kind"] > 0
        assert np.array_equal(info[two, 1], chosen["partition"][two]), name


def test_cases_cover_the_shapes_and_paths(encoded):
    """conditions on the inputs, not measurements: every partition, every kind and every swap path wins somewhere; the crafted blocks
    take the path they are named after"""
    names = set(encoded)
    for n in R2.CUBE_FACES:
        assert f"cube{n}_f32" in names and f"cube{n}_f16" in names
    assert {"flat20x12_f32", "flat20x12_f16", "partitions_f16", "partitions_f32", "crafted_f16", "crafted_f32", "edge_scene"} <= names
    kind = np.concatenate([c["kind"] for _, _, _, c in encoded.values()])
    part = np.concatenate([c["partition"] for _, _, _, c in encoded.values()])
    swap = np.concatenate([c["swap0"] * 1 + c["swap1"] * 2 for _, _, _, c in encoded.values()])
    assert set(kind.tolist()) == {0, 1, 2, 3, 4}, np.bincount(kind)
    assert set(part[kind > 0].tolist()) == set(range(32))
    assert set(swap[kind > 0].tolist()) == {0, 1, 2, 3}
    # the prototype of the issue met the first two on the 68^2 cube plus the scene alone
    pair = [encoded["cube68_f32"][3], encoded["edge_scene"][3]]
    kind2 = np.concatenate([c["kind"] for c in pair])
    part2 = np.concatenate([c["partition"] for c in pair])
    assert set(kind2.tolist()) == {0, 1, 2, 3, 4} and set(part2[kind2 > 0].tolist()) == set(range(32))

    strip = encoded["partitions_f16"][3]
    assert (strip["kind"][:32] == 0).all()                                    # two flat colours: a tie, the one-region block stays
    assert (strip["kind"][32:] > 0).all() and np.array_equal(strip["partition"][32:], np.arange(32))

    for case in ("crafted_f16", "crafted_f32"):
        _, h, _, c = encoded[case]
        at = {n: i for i, n in enumerate(R2.CRAFTED_NAMES)}

        def chose(name):
            i = at[name]
            return int(c["kind"][i]), int(c["partition"][i]), bool(c["swap0"][i]), bool(c["swap1"][i])

        assert chose("no_swap")[1:] == (13, False, False) and chose("no_swap")[0] > 0
        assert chose("swap0")[1:] == (13, True, False) and chose("swap0")[0] > 0
        assert chose("swap1_anchor15")[1:] == (13, False, True) and D.ANCHOR[13] == 15
        assert chose("swap1_anchor2")[1:] == (17, False, True) and D.ANCHOR[17] == 2
        assert chose("swap1_anchor8")[1:] == (18, False, True) and D.ANCHOR[18] == 8
        assert chose("swap_both")[1:] == (13, True, True)
        assert chose("equal_subset")[1] == 13 and chose("equal_subset")[0] > 0
        assert chose("zero")[0] == 0 and c["err"][at["zero"]] == 0
        assert chose("spread15_at10")[:2] == (1, 13) and chose("spread16_at10")[:2] == (2, 13)        # case 0 kept / left for case 14
        assert chose("spread31_at7")[:2] == (3, 13) and chose("spread32_at7")[:2] == (4, 13)          # case 1 kept / left for case 30
        for name, x0, x3, epb in (("spread15_at10", 500, 515, 10), ("spread16_at10", 500, 516, 10), ("spread31_at7", 20, 51, 7), ("spread32_at7", 20, 52, 7)):
            q = R2.quantize(R.scale(h[at[name]]), epb)                        # the texels sit on the codes of that width
            assert q[..., 0].min() == x0 and q[..., 0].max() == x3, name
        assert chose("max_next_to_small")[0] == 4                             # 65504 next to 0.2: only 6 bits span it
        for name, want_kind in (("max_at10", 1), ("max_at9", 2), ("max_at7", 3)):
            i = at[name]
            assert chose(name)[0] == want_kind and h[i].max() == R.MAX_CODE, name
            assert D.decode(encoded[case][2][i:i + 1]).max() == R.MAX_CODE    # the all-ones endpoint at that width decodes to 65504


def test_independent_decoder_reproduces_the_reported_error_and_no_inf(encoded):
    """bc6h_decode_ref knows nothing of the encoder: the squared difference of what it decodes to the source half codes is the error
    the search reported, block by block, so the bits hold what was chosen (fields, deltas, partition, anchors, swaps)"""
    for name, (_, h, blocks, chosen) in encoded.items():
        dec = D.decode(blocks)
        assert dec.max() <= R.MAX_CODE and dec.min() >= 0, name               # never Inf (0x7C00) or above
        assert np.array_equal(((dec - h) ** 2).sum(axis=(1, 2)), chosen["err"]), name
        modes = D.modes_of(blocks)
        want_mode = np.array([3, 0, 14, 1, 30])[chosen["kind"]]
        assert np.array_equal(modes, want_mode), name


def test_error_is_never_above_the_one_region_encoder(encoded):
    """per block, by construction: a two-region block replaces the one-region block only when strictly better"""
    for name, (lvl, h, blocks, chosen) in encoded.items():
        e1 = ((R.decode(R.encode(lvl)) - h) ** 2).sum(axis=(1, 2))
        assert (chosen["err"] <= e1).all(), (name, int((chosen["err"] > e1).sum()))
        one = chosen["kind"] == 0
        assert np.array_equal(chosen["err"][one], e1[one]) and np.array_equal(blocks[one], R.encode(lvl)[one]), name
        assert (chosen["err"][~one] < e1[~one]).all(), name


def test_edge_scene_error_against_the_one_region_encoder(encoded):
    """the issue's bound: below 0.75 of bc6h_ref.encode's squared half-code error on edge_scene(128) (its prototype: 0.57)"""
    lvl, h, blocks, chosen = encoded["edge_scene"]
    e2 = int(((D.decode(blocks) - h) ** 2).sum())
    e1 = int(((R.decode(R.encode(lvl)) - h) ** 2).sum())
    print("edge_scene(128): two regions", e2, "one region", e1, "ratio", e2 / e1, "kinds", np.bincount(chosen["kind"], minlength=5).tolist())
    assert e2 < 0.75 * e1


def test_quantiser_takes_the_nearest_code_at_every_width():
    """against a search over every code: nearest, the lower on a tie"""
    for epb in R2.EPB:
        u = D.unquantize(np.arange(1 << epb), epb)
        for s0 in range(0, 65536, 4096):
            s = np.arange(s0, s0 + 4096)
            assert np.array_equal(R2.quantize(s, epb), np.abs(u[None, :] - s[:, None]).argmin(axis=1)), (epb, s0)
    s = np.arange(0, 65536)
    assert np.array_equal(R2.quantize(s, 10), R.quantize(s))                  # and at 10 bits it is the one-region quantiser
