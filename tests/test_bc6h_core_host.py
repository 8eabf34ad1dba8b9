"""csrc/bc6h_core.h -- the encode rules the K18 kernel is made of -- compiled for the host (tests/bc6h_encode_host.cpp at quality 0), plain
and with ASan + UBSan, against the numpy restatement (tests/bc6h_ref.py), byte for byte; the restatement's decoder against what an independent
decoder (Pillow) recorded in tests/golden/bc6h_pillow.npz (tools/gen_bc6h_golden.py); and the properties of the contract.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bc6h_host_build  # noqa: E402
import bc6h_ref as R  # noqa: E402
from bc6h_host_build import CSRC  # noqa: E402


@pytest.fixture(scope="module", params=bc6h_host_build.VARIANTS)
def host(request, tmp_path_factory):
    return bc6h_host_build.build("bc6h_encode_host.cpp", request.param, tmp_path_factory)


@pytest.fixture(scope="module")
def encoded():
    """name -> (level, blocks of the contract): computed once, never written to"""
    out = {}
    for name, lvl in R.cases():
        blocks = R.encode(lvl)
        blocks.setflags(write=False)
        out[name] = (lvl, blocks)
    return out


def run_host(exe, tmp_path, level):
    layers, h, w, _ = level.shape
    src, dst = str(tmp_path / "texels.bin"), str(tmp_path / "blocks.bin")
    level.tofile(src)
    r = subprocess.run([exe, "0", "0" if level.dtype == np.float32 else "1", str(w), str(h), str(layers), src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    return np.fromfile(dst, np.uint8).reshape(-1, 16)


def test_bc6h_core_header_exists():
    assert os.path.isfile(os.path.join(CSRC, "bc6h_core.h")) and os.path.isfile(os.path.join(CSRC, "bc6h_format.h"))


def test_host_build_of_the_encode_core_equals_the_restatement(host, tmp_path, encoded):
    for name, (lvl, want) in encoded.items():
        got = run_host(host, tmp_path, lvl)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        bad = np.argwhere((got != want).any(axis=1)).ravel()
        assert len(bad) == 0, (name, len(bad), bad[:5].tolist(), got[bad[:1]].tolist(), want[bad[:1]].tolist())


def test_cases_cover_the_shapes_and_paths():
    names = [n for n, _ in R.cases()]
    for n in R.CUBE_FACES:
        assert f"cube{n}_f32" in names and f"cube{n}_f16" in names
    win32, win16 = R.winning_candidate(R.hostile_blocks()), R.winning_candidate(R.hostile_blocks_f16())
    for win in (win32, win16):
        assert win[6] == 1 and win[7] == 1 and win[8] == 2, win               # red up / blue down: candidate 2; the noisy block: the inset
    h = R.block_texels(R.half_codes(R.hostile_blocks()))
    _, idx, _ = R.encode_texels(h)
    raw = R._try(h, *R.candidates(h)[0])[2]
    assert raw[5, 0] >= 8 and idx[5, 0] < 8                                   # texel 0 the brightest: the swap path was taken
    codes = R.half_codes(R.hostile_blocks())[0, :, 0:4]                       # the first block: the specials in the red channel
    assert list(codes[0, :, 0]) == [0, 0, 0, 0x7BFF] and list(codes[1, :, 0]) == [0, 0x7BFF, 0x7BFF, 0x7BFF]   # -1 -0 NaN Inf | -Inf 1e30 65504 65520
    assert codes[2, 0, 0] == 0x7BFF and list(codes[2, 1:, 0]) == [1, 0, 1]   # 65519.99 | 6e-8 -> 1, 2^-25 -> 0 (tie to even), one ulp above -> 1


def test_conversion_equals_ieee_round_to_nearest_even():
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0, 1, 0x7FFFFF, 0x00800000, 0x33000000, 0x33000001, 0x33800000, 0x387FC000, 0x387FE000, 0x38800000, 0x477FE000, 0x477FF000,
                     0x477FEFFF, 0x47800000, 0x7F800000, 0xFF800000, 0x80000000, 0x3F801000, 0x3F803000, 0x3F801001], np.uint32)
    bits = np.concatenate([bits, edge])
    f = bits.view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        want = f.astype(np.float16).view(np.uint16).astype(np.int64)
    got = R.f16_from_f32(bits)
    ok = ~np.isnan(f)
    assert np.array_equal(got[ok], want[ok])
    assert ((got[~ok] & 0x7FFF) > 0x7C00).all()
    assert [int(R.WEIGHTS[i]) for i in range(16)] == [(i * 64 + 7) // 15 for i in range(16)]          # the header's closed form


def test_mode_bits_anchor_and_no_inf(encoded):
    for name, (lvl, blocks) in encoded.items():
        assert (blocks[:, 0] & 31 == 3).all(), name
        h = R.block_texels(R.half_codes(lvl))
        q, idx, err = R.encode_texels(h)
        assert (idx[:, 0] < 8).all() and np.array_equal(R.pack(q, idx), blocks), name
        dec = R.decode(blocks)
        assert dec.max() <= R.MAX_CODE and dec.min() >= 0, name               # never Inf (0x7C00) or above
        assert np.array_equal(((dec - h) ** 2).sum(axis=(1, 2)), err), name  # the swap kept the palette; the bits hold what was chosen
    assert np.isfinite(R.decode_level(encoded["hostile_f32"][1], 40, 4, 1)).all()
    with pytest.raises(ValueError):
        R.decode(np.zeros((1, 16), np.uint8))


def test_error_is_never_above_the_bounding_box_encoder(encoded):
    """per block, by construction: candidate 1 is the bounding box and a later candidate replaces it only when strictly better"""
    total3 = total1 = 0
    for name, (lvl, blocks) in encoded.items():
        h = R.block_texels(R.half_codes(lvl))
        e3 = ((R.decode(blocks) - h) ** 2).sum(axis=(1, 2))
        e1 = ((R.decode(R.encode_bbox(lvl)) - h) ** 2).sum(axis=(1, 2))
        assert (e3 <= e1).all(), (name, int((e3 > e1).sum()))
        total3 += int(e3.sum()); total1 += int(e1.sum())
    assert total3 < total1                                                    # and the extra candidates do win somewhere


def test_block_of_equal_texels_decodes_within_the_quantisation_step():
    """16 texels of half code h: every candidate is the point s = (64 h + 30) / 31, so 31 s / 64 - 30 / 64 <= h <= 31 s / 64.  Both
    endpoints quantise to the same x with u = unq(x); every palette entry is ((64 u + 32) >> 6) * 31 >> 6 = floor(31 u / 64) = d, so
    31 u / 64 - 1 < d <= 31 u / 64.  unq steps by 64 between x = 1 and 1022 (|u - s| <= 32) and by 96 resp. 95 at the two ends
    (|u - s| <= 48).  Hence d - h <= 31 |u - s| / 64 + 30 / 64 and h - d < 31 |u - s| / 64 + 1:
        96 <= s <= 65440:  -16 <= d - h <= 15        (15.5 + 0.47 -> 15; 15.5 + 1 -> 16)
        elsewhere:         -24 <= d - h <= 23        (23.25 + 0.47 -> 23; 23.25 + 1 -> 24)
    Measured over every code 0 .. 0x7BFF: -16 .. 14 inside, -23 .. 22 at the ends."""
    codes = np.arange(0, R.MAX_CODE + 1)
    h = np.repeat(np.repeat(codes[:, None, None], 16, axis=1), 3, axis=2)
    q, idx, _ = R.encode_texels(h)
    dec = R.decode(R.pack(q, idx))
    assert (dec == dec[:, :1, :1]).all()                                      # one value per block
    d = dec[:, 0, 0] - codes
    s = R.scale(codes)
    inner = (s >= 96) & (s <= 65440)
    print("equal blocks: inner", d[inner].min(), d[inner].max(), "ends", d[~inner].min(), d[~inner].max())
    assert d[inner].min() >= -16 and d[inner].max() <= 15
    assert d[~inner].min() >= -24 and d[~inner].max() <= 23


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "bc6h_pillow.npz"))


def test_decoder_equals_the_recorded_independent_decoder(golden):
    """floor(clamp(decode, 0, 1) * 255) within one 8-bit code of Pillow's BC6H decoder on every texel; texels above 1 (Pillow: 255)
    are part of it, they are the only ones that set an endpoint's top bit"""
    names = [n[:-len("_blocks")] for n in golden.files if n.endswith("_blocks")]
    assert sorted(names) == ["bright16", "hostile", "smooth32"]
    texels = saturated = 0
    for n in names:
        w, h = (int(v) for v in golden[n + "_size"])
        want = golden[n + "_rgb"].astype(np.int64)
        assert want.shape == (h, w, 3)
        blocks = golden[n + "_blocks"]
        dec = R.decode_level(blocks, w, h, 1)[0]
        got = np.floor(np.clip(dec, 0.0, 1.0) * 255.0).astype(np.int64)
        diff = np.abs(got - want)
        print(n, "max", int(diff.max()), "differing", int((diff > 0).sum()), "of", diff.size)
        assert diff.max() <= 1, (n, int(diff.max()), int((diff > 1).sum()))
        texels += w * h
        saturated += int((dec > 1.0).sum())
        assert (want[dec > 1.0] == 255).all(), n
    assert texels <= 64 * 64 and saturated > 100
    assert np.array_equal(golden["hostile_blocks"], R.encode(R.hostile_blocks()))       # the recorded blocks are the contract's


def test_golden_file_is_small():
    assert os.path.getsize(os.path.join(HERE, "golden", "bc6h_pillow.npz")) < 100 * 1024
