"""The BC6H_UF16 decode contract (K19) on the CPU: the numpy restatement (tests/bc6h_decode_ref.py) against what an independent decoder
(Pillow) recorded for every mode value in tests/golden/bc6h_modes_pillow.npz (tools/gen_bc6h_decode_golden.py); csrc/bc6h_decode_core.h
compiled for the host (tests/bc6h_decode_core_host.cpp), plain and with ASan + UBSan as a stand-alone program, byte for byte against the
restatement; the exact half -> float widening; PBR_DecodeBC6HBlocks of the library.  No GPU, no Pillow."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "vulkan-pbr-renderer_amd", "python"))
import bc6h_decode_ref as D  # noqa: E402
import bc6h_host_build  # noqa: E402
import bc6h_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "bc6h_modes_pillow.npz"))


@pytest.fixture(scope="module", params=bc6h_host_build.VARIANTS)
def host(request, tmp_path_factory):
    return bc6h_host_build.build("bc6h_decode_core_host.cpp", request.param, tmp_path_factory)


def run_host(exe, tmp_path, blocks, w, h, layers):
    src, dst = str(tmp_path / "blocks.bin"), str(tmp_path / "codes.bin")
    np.ascontiguousarray(blocks, np.uint8).tofile(src)
    r = subprocess.run([exe, "decode", str(w), str(h), str(layers), src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    return np.fromfile(dst, np.uint16).reshape(layers, h, w, 3)


def test_the_golden_file_holds_every_mode_value_and_is_small(golden):
    assert len(D.MODE_VALUES) == 18 and len(D.MODES) == 14
    assert sorted(golden.files) == sorted([f"mode{m}_blocks" for m in D.MODE_VALUES] + [f"mode{m}_rgb" for m in D.MODE_VALUES])
    for m in D.MODE_VALUES:
        blocks = golden[f"mode{m}_blocks"]
        assert blocks.shape == (64, 16) and golden[f"mode{m}_rgb"].shape == (32, 32, 3)
        assert (D.modes_of(blocks) == m).all(), m
    assert os.path.getsize(os.path.join(HERE, "golden", "bc6h_modes_pillow.npz")) < 100 * 1024


@pytest.mark.parametrize("mode", D.MODE_VALUES)
def test_restatement_equals_the_recorded_independent_decoder(golden, mode):
    """floor(clamp(decode, 0, 1) * 255) against Pillow's 8-bit output, per mode: within one code everywhere, equal on at least 99.5 % of
    the values; at least 15 % of a valid mode's values lie strictly inside (0, 255) -- Pillow saturates texels above 1, those carry no
    information; the reserved modes are all zero on both sides"""
    want = golden[f"mode{mode}_rgb"].astype(np.int64)
    dec = D.decode_level_codes(golden[f"mode{mode}_blocks"], 32, 32, 1)[0].view(np.float16).astype(np.float32)
    got = np.floor(np.clip(dec, 0.0, 1.0) * 255.0).astype(np.int64)
    diff = np.abs(got - want)
    equal, inside = float((diff == 0).mean()), float(((want > 0) & (want < 255)).mean())
    print(f"mode {mode}: max {int(diff.max())} equal {equal:.4f} inside {inside:.3f}")
    assert diff.max() <= 1
    assert equal >= 0.995
    if mode in D.RESERVED:
        assert not dec.any() and not want.any()
    else:
        assert inside >= 0.15


@pytest.fixture(scope="module")
def inputs(golden):
    """name -> (blocks uint8 [n][16], w, h, layers, the restatement's codes): computed once, never written to"""
    out = {}

    def add(name, blocks, w, h, layers):
        blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
        codes = D.decode_level_codes(blocks, w, h, layers)
        for a in (blocks, codes):
            a.setflags(write=False)
        out[name] = (blocks, w, h, layers, codes)

    add("golden", np.concatenate([golden[f"mode{m}_blocks"] for m in D.MODE_VALUES]), 32, 32, 18)
    add("random", np.random.default_rng(0xD6C0DE).integers(0, 256, (10000, 16), dtype=np.uint8), 400, 400, 1)
    add("zeros", np.zeros((1, 16), np.uint8), 4, 4, 1)
    add("ones", np.full((1, 16), 255, np.uint8), 4, 4, 1)
    lvl = R.hdr_level(20, 12, 2, 77)
    add("encoded_hdr", R.encode(lvl), 20, 12, 2)
    add("encoded_hdr_ragged", R.encode(R.hdr_level(7, 9, 1, 78)), 7, 9, 1)
    add("encoded_hostile", R.encode(R.hostile_blocks()), 40, 4, 1)
    return out


def test_host_build_of_the_decode_core_equals_the_restatement(host, tmp_path, inputs):
    for name, (blocks, w, h, layers, want) in inputs.items():
        got = run_host(host, tmp_path, blocks, w, h, layers)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (name, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def test_every_decoded_value_is_a_finite_half(inputs):
    for name, (_, _, _, _, codes) in inputs.items():
        assert codes.max() <= D.MAX_CODE, name
    assert inputs["random"][4].max() > 0x7000                                 # and the top of the range is reached
    assert not inputs["zeros"][4].any() and not inputs["ones"][4].any()      # mode 0 of zero endpoints; the reserved mode 31
    modes = D.modes_of(inputs["random"][0])
    assert set(np.unique(modes)) == set(D.MODE_VALUES)                        # 10^4 random blocks reach every mode value


def test_mode_3_blocks_decode_as_the_encoder_side_decoder(inputs):
    """on the encoder's own output (mode 3 throughout) the restatement is the existing bc6h_ref.decode"""
    for name in ("encoded_hdr", "encoded_hdr_ragged", "encoded_hostile"):
        blocks = inputs[name][0]
        assert (D.modes_of(blocks) == 3).all()
        assert np.array_equal(D.decode(blocks), R.decode(blocks)), name
    with pytest.raises(ValueError):
        R.decode(D.random_blocks(4, 1, mode=0))                               # which still handles nothing else


def test_widening_equals_ieee_on_every_code(host, tmp_path):
    """bc6hd_f32_from_code against numpy's float16 -> float32 on all 0x7C00 codes, the 1023 subnormal halves included"""
    dst = str(tmp_path / "widen.bin")
    r = subprocess.run([host, "widen", dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.fromfile(dst, np.uint32)
    want = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32).view(np.uint32)
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


def test_library_host_decoder_at_7x9():
    """PBR_DecodeBC6HBlocks: random modes per block, the last block column and row partial; texels outside the level are dropped"""
    import pbrhip
    blocks = D.random_blocks(2 * 3, 0x709)
    want = D.decode_level_codes(blocks, 7, 9, 1)[0]
    got = pbrhip.decode_bc6h_blocks_host(blocks, 7, 9)
    assert got.shape == (9, 7, 3) and np.array_equal(got, want)
    L = pbrhip.lib()
    L.PBR_DecodeBC6HBlocks(None, 7, 9, got.ctypes.data_as(pbrhip.C.POINTER(pbrhip.C.c_uint16)))       # nothing is done
    L.PBR_DecodeBC6HBlocks(blocks.ctypes.data_as(pbrhip.VP), 0, 9, got.ctypes.data_as(pbrhip.C.POINTER(pbrhip.C.c_uint16)))
    assert np.array_equal(got, want)
