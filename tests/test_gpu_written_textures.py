"""After an op writes a texture, nothing samples data built from its old bytes: the apron, the cells of every level, the LUT cells and
the per-level range are dropped by texture_written(), which exec_op calls for every texture op_effects() lists as written.  One
row of WRITERS per op kind that writes a sampled map: the next writer gets one row here.

A. every writer x both K5 kernels (fast: cells and LUT cells; general, pbrk_shade_set_fast(0): aprons): shade, write, shade; a fresh
   rig with the written maps' bytes, read back, gives the same frame bit for bit, and the frame moved on more than 10 % of the surface
   pixels (the cap of test_gpu_shade_edges.py::test_twins_follow_their_texture: a writer that changed nothing visible does not pass).
B. the precompute path, which asks for the cells by themselves: a K3 level from a 16^2 source level, before and after a copy onto it.
C. the range of GPUX_SetPrefilterTolerance follows the texture: the kept-sample count after a copy is a fresh texture's.
D. the writers that may be captured (GPUX_SetGraphReplay): [writer, shade] takes the plain path, the shade alone is captured after it.

The frame is the 96 x 64 / 64^2 / 32^2 / 64^2 case of that test; its maps are uploaded as data and the ShadeCase is never changed."""
import copy
import ctypes as C

import numpy as np
import pytest

import shade_maps as SM
import shade_sh_ref as SR
from gpu_rigs import ALL, ShadeRig
from shade_maps import IBL

pytestmark = pytest.mark.gpu

GENERAL, FAST = 0, 1
SEED = 0x5EED0F0E
COMPUTE = 2                                                                   # GPU_ShaderStage_Compute


@pytest.fixture(scope="module")
def case():
    return SM.ShadeCase(96, 64, 64, 32, 64)


@pytest.fixture(scope="module")
def env_tex(gpu):
    """A 64^2 environment with its chain: what the generators of the host library filter from.  Only ever read."""
    import pbrhip
    from pbrhip import synth
    tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 64, 64, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, synth.synth_env(64, seed=0x5EED00AA))
    yield tex
    gpu.GPU_WaitUntilIdle()
    gpu.GPU_DestroyTexture(tex)


class Off(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("z", C.c_int)]


class Blit(C.Structure):                                                      # GPU_OpBlitInfo [gpu.h:317-327]
    _fields_ = [("filter", C.c_int), ("src_texture", C.c_void_p), ("dst_texture", C.c_void_p), ("src_layer", C.c_uint32), ("dst_layer", C.c_uint32),
                ("src_mip_level", C.c_uint32), ("dst_mip_level", C.c_uint32), ("src_area", Off * 2), ("dst_area", Off * 2)]


class Scratch:
    """Textures, buffers and graphs a writer needs besides the rig; freed with the test."""

    def __init__(self, L):
        self.L, self.textures, self.buffers, self.graphs = L, [], [], []

    def cube(self, n, data):
        import pbrhip
        self.textures.append(pbrhip.make_texture(pbrhip.Format_RGBA32F, n, n, pbrhip.TextureFlag_Cubemap, data))
        return self.textures[-1]

    def buffer(self, nbytes, data=None, host=False):
        import pbrhip
        raw = None if data is None else np.ascontiguousarray(data).ctypes.data_as(C.c_void_p)
        self.buffers.append(self.L.GPU_MakeBuffer(int(nbytes), pbrhip.BufferFlag_CPU if host else pbrhip.BufferFlag_GPU, raw))
        assert self.buffers[-1]
        return self.buffers[-1]

    def graph(self):
        self.graphs.append(self.L.GPU_MakeGraph())
        return self.graphs[-1]

    def free(self):
        L = self.L
        L.GPU_WaitUntilIdle()
        for g in self.graphs:
            L.GPU_DestroyGraph(g)
        for b in self.buffers:
            L.GPU_DestroyBuffer(b)
        for t in self.textures:
            L.GPU_DestroyTexture(t)


def run(L, g):
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)


def texture_of(rig, which):
    return {"pre": rig.maps.tex_specular_env_map, "irr": rig.maps.irradiance_map, "lut": rig.maps.brdf_lut}[which]


def random_cube(rng, n):
    """Positive, and unlike any level of shade_maps: [6][n][n][4] float32 in [0.3, 4), alpha 1."""
    a = rng.uniform(0.3, 4.0, (6, n, n, 4)).astype(np.float32)
    a[..., 3] = 1.0
    return a


def random_level(rng, tex, level):
    t = tex.contents
    n = max(t.width >> level, 1)
    if t.layer_count == 6:
        return random_cube(rng, n)
    return rng.uniform(0.05, 0.95, (n, n, 2)).astype(np.float16)                # the RG16F LUT


# ---- the writers ----
# make(L, rig, rng, tmp, env) prepares what the writer needs and returns record(g), which records the op(s) into a graph -- or, for the
# writers that bring their own graph (the host library's generators) or none (a write behind the backend's back), apply().

def copy_of(which, level):
    def make(L, rig, rng, tmp, env):
        tex = texture_of(rig, which)
        data = random_level(rng, tex, level)
        buf = tmp.buffer(data.nbytes, data, host=True)
        return lambda g: L.GPU_OpCopyBufferToTexture(g, buf, tex, 0, tex.contents.layer_count, level)
    return make


def clear_of(which, level, rgba):
    def make(L, rig, rng, tmp, env):
        return lambda g: L.GPU_OpClearColorF(g, texture_of(rig, which), level, *rgba)
    return make


def blit_onto_level1(src_size):
    """Six blits, one per face (a blit is of one layer), from level 0 of a random cube onto level 1 (32^2) of the prefiltered cube:
    from 32^2 they are 1:1 copies, from 64^2 the 2:1 box."""
    def make(L, rig, rng, tmp, env):
        src = tmp.cube(src_size, random_cube(rng, src_size))
        dst = rig.maps.tex_specular_env_map
        blits = []
        for face in range(6):
            b = Blit(); b.filter = 0; b.src_layer = b.dst_layer = face; b.src_mip_level = 0; b.dst_mip_level = 1
            b.src_texture = C.cast(src, C.c_void_p); b.dst_texture = C.cast(dst, C.c_void_p)
            b.src_area[1] = Off(src_size, src_size, 1); b.dst_area[1] = Off(32, 32, 1)
            blits.append(b)

        def record(g):
            for b in blits:
                L.GPU_OpBlit(g, C.byref(b))
        return record
    return make


def new_level0(L, rig, rng):
    """For the mip generation: a level 0 that is not the old chain's, uploaded before the first frame."""
    rig.upload("pre0", random_cube(rng, 64))


def mipgen(L, rig, rng, tmp, env):
    return lambda g: L.GPU_OpGenerateMipmaps(g, rig.maps.tex_specular_env_map)


def bc6h_decode_level0(L, rig, rng, tmp, env):
    """Blocks of a random 64^2 level, encoded on the device into a device buffer; the writer decodes them into level 0."""
    pre = rig.maps.tex_specular_env_map
    nbytes = L.GPUX_BC6HMipBytes(pre, 0)
    assert nbytes == 6 * 16 * 16 * 16
    blocks = tmp.buffer(nbytes)
    g = tmp.graph()
    L.GPUX_OpEncodeBC6H(g, tmp.cube(64, random_cube(rng, 64)), 0, blocks, 0)
    run(L, g)
    return lambda g: L.GPUX_OpDecodeBC6H(g, blocks, 0, pre, 0)


def irradiance_from_sh9(L, rig, rng, tmp, env):
    coef = tmp.buffer(216, np.ascontiguousarray(SR.coef_positive(), np.float64).reshape(27))
    return lambda g: L.GPUX_OpIrradianceFromSH9(g, coef, 0, rig.maps.irradiance_map, 0)


def behind_the_back(L, rig, rng, tmp, env):
    """A kernel of the library's own ABI fills level 1 through the texture's device pointer: the backend sees no op."""
    def apply():
        pre = rig.maps.tex_specular_env_map
        texel = (C.c_float * 4)(7.0, 3.0, 5.0, 1.0)
        assert L.pbrk_fill_pattern(L.GPUX_TextureDevicePtr(pre, 1), L.GPUX_TextureMipBytes(pre, 1), texel, 16, None) == 0
        L.GPU_WaitUntilIdle()
        L.GPUX_InvalidateTexture(pre)
    return apply


def generator(call):
    def make(L, rig, rng, tmp, env):
        return lambda: call(L, rig, env)
    return make


class Writer:
    def __init__(self, name, make, recorded=True, before=None):
        self.name, self.make, self.recorded, self.before = name, make, recorded, before


WRITERS = [
    # onto the prefiltered cube
    Writer("pre.copy_level1", copy_of("pre", 1)),
    Writer("pre.clear_level1", clear_of("pre", 1, (5.0, 4.0, 6.0, 1.0))),
    Writer("pre.clear_all", clear_of("pre", ALL, (5.0, 4.0, 6.0, 1.0))),
    Writer("pre.blit_1to1", blit_onto_level1(32)),
    Writer("pre.blit_2to1", blit_onto_level1(64)),
    Writer("pre.mipgen", mipgen, before=new_level0),
    Writer("pre.K4_prefilter", generator(lambda L, rig, env: L.PBR_GenPrefilteredEnvMap(env, rig.maps.tex_specular_env_map, 1)), recorded=False),
    Writer("pre.bc6h_decode_level0", bc6h_decode_level0),
    Writer("pre.invalidate_after_external_write", behind_the_back, recorded=False),
    # onto the irradiance cube
    Writer("irr.K3_irradiance", generator(lambda L, rig, env: L.PBR_GenIrradianceMap(env, rig.maps.irradiance_map)), recorded=False),
    Writer("irr.sh9_irradiance", irradiance_from_sh9),
    Writer("irr.copy", copy_of("irr", 0)),
    # onto the LUT (its format takes a zero clear only: every specular term goes)
    Writer("lut.K1_brdf_lut", generator(lambda L, rig, env: L.PBR_GenBRDFIntegrationMap(rig.maps.brdf_lut)), recorded=False),
    Writer("lut.copy", copy_of("lut", 0)),
    Writer("lut.clear", clear_of("lut", 0, (0.0, 0.0, 0.0, 0.0))),
]
BY_NAME = {w.name: w for w in WRITERS}


def read_maps(rig):
    import pbrhip
    pre = rig.maps.tex_specular_env_map
    return dict(pre_levels=[pbrhip.read_mip(pre, l) for l in range(pre.contents.mip_level_count)],
                irr=pbrhip.read_mip(rig.maps.irradiance_map, 0), lut=pbrhip.read_mip(rig.maps.brdf_lut, 0))


def case_with(case, maps):
    """The same frame over other map bytes: a copy, the shared case stays as it is."""
    c = copy.copy(case)
    c.pre_levels, c.irr, c.lut, c._ref = maps["pre_levels"], maps["irr"], maps["lut"], {}
    return c


def share_changed(case, a, b):
    return float((a[..., :3] != b[..., :3]).any(-1)[case.surface].mean())


# ---- A. every writer drops every twin ----

@pytest.mark.parametrize("kernel", ["fast", "general"])
@pytest.mark.parametrize("writer", WRITERS, ids=[w.name for w in WRITERS])
def test_every_writer_drops_every_twin(gpu, case, env_tex, writer, kernel):
    L = gpu
    which = GENERAL if kernel == "general" else FAST
    rng = np.random.default_rng(SEED)
    rig, tmp, fresh = ShadeRig(L, case), Scratch(L), None
    try:
        L.pbrk_shade_set_fast(0 if kernel == "general" else -1)
        if writer.before:
            writer.before(L, rig, rng)
        first = rig.draw_api(IBL)                                             # builds every twin
        assert L.pbrk_shade_last_kernel() == which
        step = writer.make(L, rig, rng, tmp, env_tex)
        if writer.recorded:
            g = tmp.graph()
            step(g)
            run(L, g)
        else:
            step()
        after = rig.draw_api(IBL)
        assert L.pbrk_shade_last_kernel() == which
        fresh = ShadeRig(L, case_with(case, read_maps(rig)))
        want = fresh.draw_api(IBL)
        assert L.pbrk_shade_last_kernel() == which
        changed = share_changed(case, after, first)
        stale = share_changed(case, after, want)
        print(f"{writer.name} {kernel}: {100 * changed:.1f} % of the surface pixels changed, {100 * stale:.1f} % differ from a fresh rig's")
        assert np.array_equal(after.view(np.uint32), want.view(np.uint32)), (writer.name, stale)
        assert changed > 0.10, (writer.name, changed)
    finally:
        L.pbrk_shade_set_fast(-1)
        rig.destroy()
        if fresh:
            fresh.destroy()
        tmp.free()


# ---- B, C. the precompute path ----

class IblLevel:
    """One K3 / K4 dispatch over a whole level through the GPU_* calls, with a GPUX_IBLConstants block: it names the source LOD."""

    def __init__(self, L, shader, out, out_mip, constants):
        import pbrhip
        self.L, self.out, self.out_mip = L, out, out_mip
        self.constants = pbrhip.GPUX_IBLConstants(*constants)
        self.layout = L.GPU_InitPipelineLayout()
        self.b_sampler = L.GPU_SamplerBinding(self.layout, b"SAMPLER_LINEAR_CLAMP")
        self.b_env = L.GPU_TextureBinding(self.layout, b"TEX_ENV_CUBE")
        self.b_out = L.GPU_StorageImageBinding(self.layout, b"OUTPUT", pbrhip.Format_RGBA32F)
        L.GPU_FinalizePipelineLayout(self.layout)
        desc, errs = pbrhip.GPU_ShaderDesc(), pbrhip.GPU_GLSLErrorArray()
        desc.glsl_debug_filepath = pbrhip.GPU_String(shader, len(shader))
        desc.spirv = L.GPU_SPIRVFromGLSL(None, COMPUTE, self.layout, C.byref(desc), C.byref(errs))
        assert desc.spirv.length > 0 and errs.length == 0
        self.pipe = L.GPU_MakeComputePipeline(self.layout, C.byref(desc))
        assert self.pipe
        self.g = L.GPU_MakeGraph()

    def run(self, env):
        """A graph whose first (and only) op is the dispatch -> the output level."""
        import pbrhip
        L = self.L
        s = L.GPU_InitDescriptorSet(None, self.layout)
        L.GPU_SetSamplerBinding(s, self.b_sampler, L.GPU_SamplerLinearClamp())
        L.GPU_SetTextureBinding(s, self.b_env, env)
        L.GPU_SetStorageImageBinding(s, self.b_out, self.out, self.out_mip)
        L.GPU_FinalizeDescriptorSet(s)
        L.GPU_OpBindComputePipeline(self.g, self.pipe)
        L.GPU_OpBindComputeDescriptorSet(self.g, s)
        L.GPU_OpPushComputeConstants(self.g, self.layout, C.byref(self.constants), C.sizeof(self.constants))
        L.GPUX_OpDispatchRows(self.g, 0, 6, 0, max(self.out.contents.width >> self.out_mip, 1))
        run(L, self.g)
        L.GPU_DestroyDescriptorSet(s)
        return pbrhip.read_mip(self.out, self.out_mip).copy()

    def destroy(self):
        L = self.L
        L.GPU_WaitUntilIdle()
        L.GPU_DestroyGraph(self.g); L.GPU_DestroyComputePipeline(self.pipe); L.GPU_DestroyPipelineLayout(self.layout)


def env32(level0, level1=None):
    """A 32^2 environment with its chain, optionally with other bytes copied onto level 1 (16^2)."""
    import pbrhip
    tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 32, 32, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, level0)
    if level1 is not None:
        pbrhip.upload_mip(tex, 1, level1)
    return tex


def test_precompute_level_follows_a_copy_onto_its_source(gpu):
    """K3 from source level 1 (16^2, sampled through the apron and the cells of that level) of a 32^2 environment; a copy onto level 1;
    the same dispatch first in its graph: the output is a fresh environment texture's with those bytes, and not the one before."""
    import pbrhip
    L = gpu
    rng = np.random.default_rng(SEED + 1)
    level0, level1 = random_cube(rng, 32), random_cube(rng, 16)
    out = pbrhip.make_texture(pbrhip.Format_RGBA32F, 8, 8, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_StorageImage)
    k3 = IblLevel(L, b"gen_irradiance_map.glsl", out, 0, (0, 0.0, 1.0, 0))       # src_lod 1, the default 1024 samples
    env, fresh = env32(level0), env32(level0, level1)
    try:
        before = k3.run(env)
        pbrhip.upload_mip(env, 1, level1)
        after = k3.run(env)
        want = k3.run(fresh)
        assert np.array_equal(after.view(np.uint32), want.view(np.uint32))
        assert not np.array_equal(after, before)
    finally:
        k3.destroy()
        for t in (env, fresh, out):
            L.GPU_DestroyTexture(t)


def test_prefilter_range_follows_a_copy_onto_its_source(gpu):
    """GPUX_SetPrefilterTolerance cuts a K4b table by the {min, max} of the source level.  Level 1 of the environment goes from one
    octave of range to six decades: the kept-sample count of mip 1 (roughness 0.03, 1389 samples in its table) after the copy is the
    count a fresh texture with those bytes gives, and larger than before (the bound tail * max <= rel * head * min got 1e6 / 2 harder
    to meet and the weights fall geometrically, about exp(-i / 14.7))."""
    import pbrhip
    L = gpu
    rng = np.random.default_rng(SEED + 2)
    level0 = rng.uniform(1.0, 2.0, (6, 32, 32, 4)).astype(np.float32)
    level1 = np.power(10.0, rng.uniform(-3.0, 3.0, (6, 16, 16, 4))).astype(np.float32)
    spec = pbrhip.make_texture(pbrhip.Format_RGBA32F, 16, 16, pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps | pbrhip.TextureFlag_StorageImage)
    k4b = IblLevel(L, b"gen_prefiltered_env_map.glsl", spec, 1, (1, 0.03, 1.0, 0))    # mip 1 from src_lod 1, the default 8192 samples
    env, fresh = env32(level0), env32(level0, level1)
    try:
        L.GPUX_SetPrefilterTolerance(1e-7)
        k4b.run(env)
        narrow = L.GPUX_PrefilterKeptSamples(1)
        pbrhip.upload_mip(env, 1, level1)
        k4b.run(env)
        after = L.GPUX_PrefilterKeptSamples(1)
        k4b.run(fresh)
        want = L.GPUX_PrefilterKeptSamples(1)
        print(f"kept samples of mip 1: {narrow} over one octave, {after} after the copy, {want} on a fresh texture")
        assert after == want
        assert 0 < narrow < after <= 1389
    finally:
        L.GPUX_SetPrefilterTolerance(0.0)
        k4b.destroy()
        for t in (env, fresh, spec):
            L.GPU_DestroyTexture(t)


# ---- D. replay ----

def replay_launches(L, g):
    s = [C.c_uint64() for _ in range(3)]
    L.GPUX_GraphReplayStats(g, *[C.byref(v) for v in s])
    return s[0].value


# the writer kinds that may be captured (op_replayable): a clear with a one-launch texel size, mipgen, a 1:1 blit, SH9 irradiance, BC6H decode
CAPTURABLE = ["pre.clear_level1", "pre.mipgen", "pre.blit_1to1", "irr.sh9_irradiance", "pre.bc6h_decode_level0"]


@pytest.mark.parametrize("name", CAPTURABLE)
def test_writer_in_front_of_a_shade_is_not_captured(gpu, case, env_tex, name):
    """[writer of a map the shade samples, shade] under GPUX_SetGraphReplay(1): the shade would rebuild its twins inside the capture,
    so the graph takes the plain path (the launch count of GPUX_GraphReplayStats does not move) and its frame is the one with replay
    off; before each of the two runs the maps are the case's again and shaded, so a stale twin would show.  The same shade alone is
    captured afterwards."""
    L = gpu
    writer = BY_NAME[name]
    rng = np.random.default_rng(SEED + 3)
    rig, tmp = ShadeRig(L, case), Scratch(L)

    def old_maps():
        for l, lv in enumerate(case.pre_levels):
            rig.upload(f"pre{l}", lv)
        rig.upload("irr", case.irr)
        if writer.before:
            writer.before(L, rig, np.random.default_rng(SEED + 4))           # the same level 0 both times
        return rig.draw_api(IBL)

    def record_shade():
        L.GPUX_SetShadeFlags(L.PBR_LightingPipeline(rig.lp), IBL)
        L.PBR_RecordLightingPass(rig.lp, rig.g, C.byref(case.glob), 0, 0)

    try:
        L.GPUX_EnableOpTiming(0)                                              # per-op timing keeps every graph on the plain path
        frames = []
        step = None
        for replay in (0, 1):
            L.GPUX_SetGraphReplay(0)
            old = old_maps()
            step = step or writer.make(L, rig, rng, tmp, env_tex)
            L.GPUX_SetGraphReplay(replay)
            launches = replay_launches(L, rig.g)
            step(rig.g)
            record_shade()
            run(L, rig.g)
            assert replay_launches(L, rig.g) == launches, f"{name}: captured with replay {replay}"
            frames.append(rig.read())
            assert not np.array_equal(frames[-1], old)
        assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))
        L.GPUX_SetGraphReplay(1)
        launches = replay_launches(L, rig.g)
        record_shade()
        run(L, rig.g)
        assert replay_launches(L, rig.g) == launches + 1
        assert np.array_equal(rig.read().view(np.uint32), frames[0].view(np.uint32))
    finally:
        L.GPUX_SetGraphReplay(-1)
        rig.destroy()
        tmp.free()
