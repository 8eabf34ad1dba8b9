"""BC materials through the passes that sample them: a K13 scene and a K14 scene drawn once with BC1 / BC5 / BC3 material textures and
once with RGBA8UN one-level twins uploaded from the numpy restatement of the decode (tests/bc_decode_ref.py).  Every target must be
byte-identical between the two draws (tolerance 0: the kernels see the same RGBA8 texels either way).  And the .dds loader: files
written from the golden blocks, loaded with and without their levels, compared with the restatement and drawn with.
Textures are at most 64 x 64, frames 64 x 48, a few hundred triangles."""
import os
import struct

import numpy as np
import pytest

import bc_decode_ref as R
import voxelize_scenes as S
from geometry_scenes import random_scene
from gpu_rigs import GeometryRig as GeoRig, VoxelizeRig as VoxRig, gpu_format

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu

SLOT_FORMATS = ("bc1_rgba", "bc5", "bc3", "bc1_rgb")          # base colour (transparent texels meet the alpha test), normal, ORM, emissive


def bc_material_specs():
    """two materials of random blocks: 32 x 32, and 28 x 20 (no power of two); [(fmt, w, h, blocks)] per slot"""
    return [[(fmt, w, h, R.random_blocks(fmt, w, h, 9000 + 10 * k + s)) for s, fmt in enumerate(SLOT_FORMATS)]
            for k, (w, h) in enumerate(((32, 32), (28, 20)))]


class Materials:
    """PBR_Materials over caller-owned textures: the BC textures themselves, or their RGBA8UN twins"""

    def __init__(self, L, specs, twins):
        import pbrhip
        self.L, self.textures, self.mats = L, [], []
        for spec in specs:
            tex = []
            for fmt, w, h, blocks in spec:
                if twins:
                    tex.append(pbrhip.make_texture(pbrhip.Format_RGBA8UN, w, h, 0, R.decode(fmt, blocks, w, h)))
                else:
                    tex.append(pbrhip.make_texture(gpu_format(fmt), w, h, 0, blocks))
            self.textures += tex
            self.mats.append(pbrhip.make_material_from_textures(tex))

    def destroy(self):
        for t in self.textures:
            self.L.GPU_DestroyTexture(t)


def draw_geometry(L, scene, specs, twins, mats=None):
    m = mats or Materials(L, specs, twins)
    rig = GeoRig(L, scene, m.mats)
    g = L.GPU_MakeGraph()
    rig.clear_colour(g)
    rig.record(g)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    got = rig.read()
    L.GPU_DestroyGraph(g)
    rig.destroy()                                                             # destroys the materials (not their textures)
    if mats is None:
        m.destroy()
    return got


def same_targets(name, a, b):
    for key in ("base", "nrm", "orm", "emi", "vel", "depth"):
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[x.dtype.itemsize]
        bad = int((x.view(bits) != y.view(bits)).sum())
        print(f"{name}: {key}: {bad} differing values / tolerance 0 (bit-identical)")
        assert bad == 0, (name, key, bad)


@pytest.fixture(scope="module")
def geo_scene():
    return random_scene(64, 48, 300, seed=0x5EED1501)                      # two draws, materials 0 and 1


def test_geometry_pass_with_bc_materials_equals_rgba8_twins(gpu, geo_scene):
    specs = bc_material_specs()
    bc = draw_geometry(gpu, geo_scene, specs, twins=False)
    tw = draw_geometry(gpu, geo_scene, specs, twins=True)
    same_targets("K13 BC vs RGBA8UN twins", bc, tw)
    covered = bc["depth"] < 1.0
    assert covered.mean() > 0.3                                               # the scene covers the frame ...
    assert len(np.unique(bc["emi"][covered].reshape(-1, 4), axis=0)) > 50     # ... with textured, not constant, colour
    base = R.decode(*[specs[0][0][i] for i in (0, 3)], specs[0][0][1], specs[0][0][2])
    assert (base[..., 3] == 0).mean() > 0.05                                  # and the base colour has punch-through texels for the alpha test


def test_voxelize_pass_with_bc_materials_equals_rgba8_twins(gpu):
    scene = S.random_scene(64, 200, seed=0x5EED1502)
    specs = bc_material_specs()
    grids = []
    for twins in (False, True):
        m = Materials(gpu, specs, twins)
        rig = VoxRig(gpu, scene, m.mats)
        g = gpu.GPU_MakeGraph()
        rig.record(g)
        gpu.GPU_GraphSubmit(g); gpu.GPU_GraphWait(g)
        grids.append(rig.read())
        gpu.GPU_DestroyGraph(g)
        rig.destroy()
        m.destroy()
    a, b = (np.ascontiguousarray(x).view(np.uint16) for x in grids)
    bad = int((a != b).sum())
    print(f"K14 BC vs RGBA8UN twins: {bad} differing halfs of {a.size} / tolerance 0 (bit-identical)")
    assert bad == 0
    assert (a.reshape(-1, 4)[:, :3] != 0).any(1).sum() > 500                  # voxels were written, with colour


# ---- the .dds loader ----
def golden():
    return np.load(os.path.join(HERE, "golden", "bc_crops.npz"))


def dds_file(fourcc, w, h, levels, dx10=None):
    """a .dds around `levels` (bytes per level, largest first): legacy FourCC header, or DX10 with the given DXGI format"""
    pf = struct.pack("<II4sIIIII", 32, 0x4, b"DX10" if dx10 else fourcc, 0, 0, 0, 0, 0)
    head = struct.pack("<IIIIIII", 124, 0x1007 | (0x20000 if len(levels) > 1 else 0), h, w, len(levels[0]), 0, len(levels)) + bytes(44) + pf + \
        struct.pack("<IIIII", 0x1000 | (0x400008 if len(levels) > 1 else 0), 0, 0, 0, 0)
    ext = struct.pack("<IIIII", dx10, 3, 0, 1, 0) if dx10 else b""
    return b"DDS " + head + ext + b"".join(bytes(l) for l in levels)


def test_dds_file_loads_level_0_like_the_reference_and_all_levels_on_request(gpu, tmp_path):
    import pbrhip
    z = golden()
    # a 64 x 64 DXT1 file: level 0 = a real crop, 32 .. 16 = random blocks, 8 .. 1 = the real tail levels of the same file
    levels = [z["basecolor64_blocks"], R.random_blocks("bc1_rgba", 32, 32, 1), R.random_blocks("bc1_rgba", 16, 16, 2)] + [z[f"tail{s}_blocks"] for s in (8, 4, 2, 1)]
    path = tmp_path / "base.dds"
    path.write_bytes(dds_file(b"DXT1", 64, 64, levels))
    info = pbrhip.parse_dds(path.read_bytes())
    assert (info.format, info.width, info.height, info.level_count) == (pbrhip.Format_BC1_RGBA_UN, 64, 64, 7)
    one = pbrhip.make_texture_from_dds_file(str(path), 0)
    full = pbrhip.make_texture_from_dds_file(str(path), pbrhip.PBR_DDS_FILE_MIPS)
    try:
        assert (one.contents.format, one.contents.width, one.contents.height, one.contents.mip_level_count) == (pbrhip.Format_BC1_RGBA_UN, 64, 64, 1)
        assert (full.contents.format, full.contents.width, full.contents.height, full.contents.mip_level_count) == (pbrhip.Format_BC1_RGBA_UN, 64, 64, 7)
        assert np.array_equal(pbrhip.read_decoded_mip(one, 0), z["basecolor64_rgba"])           # what Pillow made of the same blocks
        for m, blocks in enumerate(levels):
            s = 64 >> m
            assert np.array_equal(pbrhip.read_decoded_mip(full, m), R.decode("bc1_rgba", blocks, s, s)), m
            assert pbrhip.read_mip_bytes(full, m) == bytes(blocks)
        for s in (8, 4, 2, 1):
            assert np.array_equal(pbrhip.read_decoded_mip(full, 6 - int(np.log2(s))), z[f"tail{s}_rgba"])
    finally:
        gpu.GPU_DestroyTexture(one); gpu.GPU_DestroyTexture(full)
    # the other containers: DXT5, ATI2, DX10 / DXGI 83, and a level count the chain needs but the file lacks
    for name, fmt, fourcc, dx10, want in (("rand_bc3", "bc3", b"DXT5", None, pbrhip.Format_BC3_RGBA_UN), ("rand_bc5", "bc5", b"ATI2", None, pbrhip.Format_BC5_UN),
                                          ("rand_bc5", "bc5", None, 83, pbrhip.Format_BC5_UN)):
        p = tmp_path / (name + ".dds")
        p.write_bytes(dds_file(fourcc, 32, 32, [z[name + "_blocks"]], dx10))
        t = pbrhip.make_texture_from_dds_file(str(p), pbrhip.PBR_DDS_FILE_MIPS)     # a one-level file stays a one-level texture
        try:
            assert (t.contents.format, t.contents.mip_level_count) == (want, 1)
            got, rec = pbrhip.read_decoded_mip(t, 0), z[name + "_rgba"]
            assert np.array_equal(got[..., :2], rec[..., :2]) if fmt == "bc5" else np.array_equal(got, rec)
            assert np.array_equal(got, R.decode(fmt, z[name + "_blocks"], 32, 32))
        finally:
            gpu.GPU_DestroyTexture(t)
    short = tmp_path / "short.dds"
    short.write_bytes(dds_file(b"DXT1", 64, 64, levels[:3]))
    assert not gpu.PBR_MakeTextureFromDDSFile(os.fsencode(str(short)), pbrhip.PBR_DDS_FILE_MIPS)
    assert not gpu.PBR_MakeTextureFromDDSFile(os.fsencode(str(tmp_path / "missing.dds")), 0)


def test_dds_file_wider_than_high_uploads_the_levels_of_the_smaller_extent(gpu):
    """a 64 x 16 DXT1 file holds the 7 levels of its larger extent; the texture's chain is counted from the smaller one: 5 levels, each
    the file's; the same file cut below those 5 is refused"""
    import pbrhip
    levels = [R.random_blocks("bc1_rgba", max(1, 64 >> m), max(1, 16 >> m), 700 + m) for m in range(7)]
    data = dds_file(b"DXT1", 64, 16, levels)
    assert pbrhip.parse_dds(data).level_count == 7
    t = gpu.PBR_MakeTextureFromDDSMemory(data, len(data), pbrhip.PBR_DDS_FILE_MIPS)
    assert t
    try:
        assert (t.contents.format, t.contents.width, t.contents.height, t.contents.mip_level_count) == (pbrhip.Format_BC1_RGBA_UN, 64, 16, 5)
        for m in range(5):
            assert pbrhip.read_mip_bytes(t, m) == bytes(levels[m]), m
            assert np.array_equal(pbrhip.read_decoded_mip(t, m), R.decode("bc1_rgba", levels[m], 64 >> m, max(1, 16 >> m))), m
    finally:
        gpu.GPU_DestroyTexture(t)
    cut = dds_file(b"DXT1", 64, 16, levels[:4])
    assert pbrhip.parse_dds(cut).level_count == 4
    assert not gpu.PBR_MakeTextureFromDDSMemory(cut, len(cut), pbrhip.PBR_DDS_FILE_MIPS)


def test_material_from_dds_files_draws_like_its_rgba8_twin(gpu, geo_scene, tmp_path):
    """base colour and emissive from .dds files with all their levels (the sampler walks the decoded chain), normal and ORM left NULL:
    the reference's 1 x 1 dummies.  The twin: RGBA8UN textures whose every level is uploaded from the restatement."""
    import pbrhip
    L = gpu
    z = golden()
    chains = {}
    for slot, key in (("base", "basecolor64_blocks"), ("emi", "emissive64_blocks")):
        chains[slot] = [z[key]] + [R.random_blocks("bc1_rgba", 64 >> m, 64 >> m, 300 + m + (10 if slot == "emi" else 0)) for m in range(1, 7)]
        (tmp_path / (slot + ".dds")).write_bytes(dds_file(b"DXT1", 64, 64, chains[slot]))
    results = []
    for twins in (False, True):
        tex = {}
        for slot in ("base", "emi"):
            if not twins:
                tex[slot] = pbrhip.make_texture_from_dds_file(str(tmp_path / (slot + ".dds")), pbrhip.PBR_DDS_FILE_MIPS)
            else:
                tex[slot] = pbrhip.make_texture(pbrhip.Format_RGBA8UN, 64, 64, pbrhip.TextureFlag_HasMipmaps, None)
                for m, blocks in enumerate(chains[slot]):
                    pbrhip.upload_mip(tex[slot], m, R.decode("bc1_rgba", blocks, 64 >> m, 64 >> m))
        mats = [pbrhip.make_material_from_textures([tex["base"], None, None, tex["emi"]]) for _ in range(2)]
        for k, want in enumerate(((255, 255, 255, 255), (127, 127, 255, 255), (0, 0, 0, 0), (0, 0, 0, 0))):
            t = L.PBR_MaterialTexture(mats[0], k)
            if k in (1, 2):
                assert (t.contents.width, t.contents.height, t.contents.format) == (1, 1, pbrhip.Format_RGBA8UN)
                assert tuple(pbrhip.read_mip(t, 0).ravel()) == want
        holder = type("M", (), {"mats": mats})()
        results.append(draw_geometry(L, geo_scene, None, twins, mats=holder))
        for t in tex.values():
            L.GPU_DestroyTexture(t)
    same_targets("K13 .dds material vs RGBA8UN twin", results[0], results[1])
    covered = results[0]["depth"] < 1.0
    assert len(np.unique(results[0]["base"][covered].reshape(-1, 4), axis=0)) > 50
