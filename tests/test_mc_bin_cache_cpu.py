"""The bin cache's index arithmetic (k_mc_region.hip, header 2m) on the host: pbrk_mc_tile_of_block, the twin of the kernels' block -> tile
map (mc_tile_of_block, k_mc_internal.h: plain block order but for faces +-X, whose tile rows are dealt outwards from the pole row of the
tangent frame), and pbrk_mc_bin_window_eligible, the rule that says which row windows of the region kernel have the tiles of the
whole-level dispatch.  A recorded entry is indexed [face][tile row from row 0 of the face][tile column]: a replaying dispatch must reach,
for each of its tiles, the index the whole-face dispatch gave that tile.  No GPU."""
import ctypes as C

import pytest

SIZES = (256, 250, 512)
TILES = (8, 16, 32)


@pytest.fixture(scope="module")
def L():
    import pbrhip
    return pbrhip.lib()                                       # binds the symbols; no GPU call


def tiles_of(L, size, tile, face0, nfaces, y0, y1):
    """[(face, tx, ty, index)] for every block of the dispatch, in block order."""
    tx, ty = -(-size // tile), -(-(y1 - y0) // tile)
    out, res = (C.c_int * 4)(), []
    for b in range(tx * ty * nfaces):
        assert L.pbrk_mc_tile_of_block(b, size, tile, face0, nfaces, y0, y1, out) == 0
        res.append(tuple(out))
    assert L.pbrk_mc_tile_of_block(tx * ty * nfaces, size, tile, face0, nfaces, y0, y1, out) != 0      # one block too many
    return res


def windows(size, tile):
    """Row windows that start at a multiple of the tile and end at one or at the face's end: the whole face, its halves at a tile row,
    one tile row around each pole of faces +-X (a quarter and three quarters of the height), the last (possibly clipped) tile row."""
    n = -(-size // tile)
    mid = (n // 2) * tile
    cuts = {(0, size), (0, mid), (mid, size), ((n - 1) * tile, size)}
    for frac in (0.248, 0.752):                                # the pole rows of +X / -X
        r = int(frac * size) // tile * tile
        cuts.add((r, min(r + tile, size)))
        cuts.add((r, size))
    return sorted(c for c in cuts if c[0] < c[1])


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("size", SIZES)
def test_blocks_map_one_to_one_onto_the_tiles_and_to_the_whole_face_index(L, size, tile):
    n = -(-size // tile)
    whole = {(f, tx, ty): i for f, tx, ty, i in tiles_of(L, size, tile, 0, 6, 0, size)}
    assert len(whole) == 6 * n * n and sorted(whole.values()) == list(range(6 * n * n))
    for (f, tx, ty), i in whole.items():
        assert i == (f * n + ty) * n + tx
    for y0, y1 in windows(size, tile):
        assert L.pbrk_mc_bin_window_eligible(size, tile, y0, y1) == 1, (y0, y1)
        rows = -(-(y1 - y0) // tile)
        # all six faces; +X and -X alone (the pole dealing); a face without it
        for face0, nfaces in ((0, 6), (0, 1), (1, 1), (0, 2), (4, 1)):
            got = tiles_of(L, size, tile, face0, nfaces, y0, y1)
            keys = {(f, tx, ty) for f, tx, ty, _ in got}
            want = {(f, tx, ty) for f in range(face0, face0 + nfaces) for tx in range(n) for ty in range(rows)}
            assert keys == want and len(got) == len(want), (size, tile, y0, y1, face0, nfaces)
            for f, tx, ty, i in got:
                assert i == whole[(f, tx, y0 // tile + ty)], (size, tile, y0, y1, f, tx, ty)


def test_pole_rows_come_first_on_the_x_faces(L):
    """256^2, 16 x 16 tiles, whole faces: the first tile row dealt on +X is the pole's (row 63: tile row 3), on -X row 192's (12), and
    the rows then alternate outwards; the other faces keep row order."""
    got = tiles_of(L, 256, 16, 0, 6, 0, 256)
    per_face = [got[f * 256:(f + 1) * 256] for f in range(6)]
    for f, first in ((0, 3), (1, 12)):
        order = [ty for _, tx, ty, _ in per_face[f] if tx == 0]
        assert order[0] == first and sorted(order) == list(range(16))
        assert {order[1], order[2]} == {first - 1, first + 1}
    for f in range(2, 6):
        assert [ty for _, tx, ty, _ in per_face[f] if tx == 0] == list(range(16))


@pytest.mark.parametrize("tile", (16, 32))
def test_eligibility_is_exactly_tile_start_and_tile_or_face_end(L, tile):
    for size in SIZES:
        for y0 in range(0, size, 5 if size > 256 else 1):
            for y1 in list(range(y0 + 1, size + 1, 7)) + [size]:
                want = y0 % tile == 0 and (y1 % tile == 0 or y1 == size)
                assert L.pbrk_mc_bin_window_eligible(size, tile, y0, y1) == int(want), (size, tile, y0, y1)
    # the ragged shards of the kernel-level tests
    for f in range(6):
        a, b = 5 + f, 131 - 2 * f
        assert L.pbrk_mc_bin_window_eligible(256, tile, 0, a) == 0
        assert L.pbrk_mc_bin_window_eligible(256, tile, a, b) == 0
        assert L.pbrk_mc_bin_window_eligible(256, tile, b, 256) == 0
    assert L.pbrk_mc_bin_window_eligible(256, tile, 5, 126) == 0
    # not a window at all
    for y0, y1 in ((-16, 16), (32, 32), (64, 32), (0, 272)):
        assert L.pbrk_mc_bin_window_eligible(256, tile, y0, y1) == 0


def test_bad_arguments(L):
    out = (C.c_int * 4)()
    assert L.pbrk_mc_tile_of_block(0, 256, 16, 0, 6, 0, 256, None) != 0
    assert L.pbrk_mc_tile_of_block(-1, 256, 16, 0, 6, 0, 256, out) != 0
    assert L.pbrk_mc_tile_of_block(0, 256, 12, 0, 6, 0, 256, out) != 0
    assert L.pbrk_mc_tile_of_block(0, 256, 16, 5, 2, 0, 256, out) != 0
    assert L.pbrk_mc_tile_of_block(0, 256, 16, 0, 6, 16, 16, out) != 0
    assert L.pbrk_mc_table_register(None, 10) != 0 and L.pbrk_mc_table_unregister(None) != 0
    assert L.pbrk_mc_table_unregister(C.c_void_p(0x1000)) != 0                 # never registered
