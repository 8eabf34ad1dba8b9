"""K15 on the GPU: the decoded image of BC1 / BC3 / BC5 textures against the numpy restatement (tests/bc_decode_ref.py), bit for bit,
for every format and extent of the CPU tests; the compressed bytes stay what was uploaded; a mip chain filled by copies; errors.
Textures are at most 64 x 64."""
import ctypes as C

import numpy as np
import pytest

import bc_decode_ref as R
from gpu_rigs import gpu_format

pytestmark = pytest.mark.gpu


_CASES = R.cases()
_WANT = {}


def want_of(name, fmt, w, h, blocks):
    if name not in _WANT:
        _WANT[name] = R.decode(fmt, blocks, w, h)
    return _WANT[name]


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_decoded_image_equals_the_restatement_and_blocks_stay(gpu, case):
    import pbrhip
    name, fmt, w, h, blocks = case
    tex = pbrhip.make_texture(gpu_format(fmt), w, h, 0, blocks)               # level 0 is decoded before this returns
    try:
        t = tex.contents
        assert (t.width, t.height, t.mip_level_count) == (w, h, 1)
        assert gpu.GPUX_TextureMipBytes(tex, 0) == R.level_bytes(fmt, w, h)
        got = pbrhip.read_decoded_mip(tex, 0)
        want = want_of(*case)
        bad = np.argwhere(got != want)
        print(f"{name}: {len(bad)} differing bytes of {got.size} / tolerance 0 (bit-identical)")
        assert len(bad) == 0, (name, len(bad), bad[:5].tolist())
        assert pbrhip.read_mip_bytes(tex, 0) == np.asarray(blocks, np.uint8).tobytes()      # copies in and out stay format-true
    finally:
        gpu.GPU_DestroyTexture(tex)


@pytest.mark.parametrize("fmt,w,h", [("bc1_rgba", 64, 64), ("bc3", 36, 20), ("bc5", 9, 5)])
def test_mip_chain_filled_by_copies_and_one_level_rewritten(gpu, fmt, w, h):
    """HasMipmaps without data; every level arrives by a copy op in ONE graph, then one level is rewritten: that level follows the new
    blocks, every other level keeps its bytes.  36 x 20 and 9 x 5 have odd levels, so levels below them start off a 16-byte boundary."""
    import pbrhip
    L = gpu
    tex = pbrhip.make_texture(gpu_format(fmt), w, h, pbrhip.TextureFlag_HasMipmaps, None)
    try:
        n = tex.contents.mip_level_count
        assert n == int(np.log2(min(w, h))) + 1
        dims = [(max(1, w >> m), max(1, h >> m)) for m in range(n)]
        blocks = [R.random_blocks(fmt, lw, lh, 7000 + m) for m, (lw, lh) in enumerate(dims)]
        for m in range(n):                                                    # nothing uploaded yet: the blocks are zero
            assert pbrhip.read_mip_bytes(tex, m) == bytes(R.level_bytes(fmt, *dims[m]))
        payload = np.concatenate(blocks)
        offs = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(int)
        buf = L.GPU_MakeBuffer(len(payload), pbrhip.BufferFlag_CPU, payload.ctypes.data_as(C.c_void_p))
        g = L.GPU_MakeGraph()
        L.GPU_OpCopyBufferToTexture(g, buf, tex, 0, 1, 0)                     # the reference's entry point for level 0
        for m in range(1, n):
            L.GPUX_OpCopyBufferToTextureMip(g, buf, int(offs[m]), tex, m)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        for m in range(n):
            got = pbrhip.read_decoded_mip(tex, m)
            assert np.array_equal(got, R.decode(fmt, blocks[m], *dims[m])), (fmt, m)
            assert pbrhip.read_mip_bytes(tex, m) == blocks[m].tobytes()
        before = [pbrhip.read_decoded_mip(tex, m) for m in range(n)]
        k = 1
        fresh = R.random_blocks(fmt, *dims[k], 7100)
        buf2 = L.GPU_MakeBuffer(len(fresh), pbrhip.BufferFlag_CPU, fresh.ctypes.data_as(C.c_void_p))
        L.GPUX_OpCopyBufferToTextureMip(g, buf2, 0, tex, k)
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
        for m in range(n):
            got = pbrhip.read_decoded_mip(tex, m)
            if m == k:
                assert np.array_equal(got, R.decode(fmt, fresh, *dims[k])) and not np.array_equal(got, before[k])
                assert pbrhip.read_mip_bytes(tex, m) == fresh.tobytes()
            else:
                assert np.array_equal(got, before[m]), (fmt, m)
                assert pbrhip.read_mip_bytes(tex, m) == blocks[m].tobytes()
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(buf); L.GPU_DestroyBuffer(buf2)
    finally:
        gpu.GPU_DestroyTexture(tex)


def test_kernel_abi_rejects_bad_arguments(gpu):
    """pbrk_bc_decode launches nothing for a bad format, extent or pointer"""
    import pbrhip
    tex = pbrhip.make_texture(pbrhip.Format_RGBA8UN, 8, 8, 0, np.zeros((8, 8, 4), np.uint8))
    p = gpu.GPUX_TextureDevicePtr(tex, 0)
    try:
        assert gpu.pbrk_bc_decode(4, p, 4, 4, p, None) != 0
        assert gpu.pbrk_bc_decode(0, p, 0, 4, p, None) != 0 and gpu.pbrk_bc_decode(0, p, 4, 16385, p, None) != 0
        assert gpu.pbrk_bc_decode(0, None, 4, 4, p, None) != 0 and gpu.pbrk_bc_decode(0, p, 4, 4, None, None) != 0
        assert gpu.pbrk_bc_decode(2, p + 8, 4, 4, p, None) != 0 and gpu.pbrk_bc_decode(0, p, 4, 4, p + 2, None) != 0
    finally:
        gpu.GPU_DestroyTexture(tex)


class _Errors:
    def __init__(self, L):
        self.L, self.msgs = L, []
        self.cb = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)(lambda m, u: self.msgs.append(m.decode()))

    def __enter__(self):
        self.L.GPUX_SetErrorHandler(C.cast(self.cb, C.c_void_p), None)
        return self

    def __exit__(self, *a):
        self.L.GPUX_SetErrorHandler(None, None)


def test_errors(gpu):
    import pbrhip
    L = gpu
    blocks = R.random_blocks("bc1_rgba", 16, 16, 1)
    with _Errors(L) as e:
        t = L.GPU_MakeTexture(pbrhip.Format_BC1_RGBA_UN, 16, 16, 1, pbrhip.TextureFlag_HasMipmaps, blocks.ctypes.data_as(C.c_void_p))
        assert not t and len(e.msgs) == 1 and "HasMipmaps with data" in e.msgs[0], e.msgs
        rgba = pbrhip.make_texture(pbrhip.Format_RGBA8UN, 16, 16, 0, np.zeros((16, 16, 4), np.uint8))
        bc = pbrhip.make_texture(pbrhip.Format_BC1_RGBA_UN, 16, 16, 0, blocks)
        buf = L.GPU_MakeBuffer(16 * 16 * 4, pbrhip.BufferFlag_CPU, None)
        small = L.GPU_MakeBuffer(16 * 16 * 4 - 4, pbrhip.BufferFlag_CPU, None)
        g = L.GPU_MakeGraph()
        for args, needle in (((rgba, 0, buf, 0), "no decoded image"), ((bc, 1, buf, 0), "bad arguments"), ((bc, 0, small, 0), "buffer too small"),
                             ((bc, 0, buf, 4), "buffer too small")):
            e.msgs.clear()
            L.GPUX_OpCopyDecodedTextureMipToBuffer(g, *args)
            assert len(e.msgs) == 1 and needle in e.msgs[0], (needle, e.msgs)
        e.msgs.clear()
        L.GPU_OpGenerateMipmaps(g, bc)                                        # a compressed chain cannot be generated
        assert len(e.msgs) == 1, e.msgs
        e.msgs.clear()
        L.GPU_OpClearColorF(g, bc, 0, 0.0, 0.0, 0.0, 0.0)
        assert len(e.msgs) == 1 and "cannot be cleared" in e.msgs[0], e.msgs
        e.msgs.clear()
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)                              # nothing was recorded
        assert e.msgs == []
        L.GPU_DestroyGraph(g); L.GPU_DestroyBuffer(buf); L.GPU_DestroyBuffer(small)
        L.GPU_DestroyTexture(rgba); L.GPU_DestroyTexture(bc)
