"""K5 with the ambient term from SH9 coefficients (PBRK_SHADE_SH9 / GPUX_Shade_SH9Irradiance, csrc/sh_shade_core.h) instead of the
irradiance cube: every instantiation at the ragged frames of shade_maps against the composite reference of shade_sh_ref.py (the
oracle's frames with a zero and a constant cube, combined with the double SH contract at each pixel's raw normal), coefficients
produced on the device in the same and in an earlier graph, hipGraph replay, the twins that are no longer built, record-time checks,
switching back, and the demo's option.

The criterion is the suite's for K5: rel_map(got, want) < 1e-4 (floor 1e-2) on the pixels the conditioning screen keeps, fp16 targets
within one code of the rounded reference.  Bit-equality checks are not screened."""
import ctypes as C
import os

import numpy as np
import pytest

import sh_ref as R
import shade_maps as SM
import shade_sh_ref as SR
from gpu_rigs import ShadeRig
from shade_maps import GI, IBL, SHADOWS, SHAFTS
from shade_sh_ref import SH9

pytestmark = pytest.mark.gpu

GENERAL, FAST, LIVE = 0, 1, 2
FLAG_SETS = ((IBL, FAST), (IBL | SHAFTS, FAST), (IBL | SHADOWS, GENERAL))     # without the SH9 bit; SH mode stays on the fast path
E_ARG = -1
_REF = {}


def reference(size, flags):
    """(case, Composite) for one ragged frame and flag set, computed once per session; the case is shared by every flag set of a size"""
    if ("case", size) not in _REF:
        _REF[("case", size)] = SR.make_case(size[0], size[1], shadows=True)
    case = _REF[("case", size)]
    if (size, flags) not in _REF:
        _REF[(size, flags)] = SR.Composite(case, flags)
    return case, _REF[(size, flags)]


def _fmt(name):
    import pbrhip
    return {"f32": pbrhip.Format_RGBA32F, "f16": pbrhip.Format_RGBA16F}[name]


def coef_buffer(L, coef, host=False, pad=0):
    """27 doubles (after `pad` bytes of 0x5A) in a device buffer, or in a mapped host buffer that the test may rewrite"""
    import pbrhip
    raw = b"\x5a" * pad + np.ascontiguousarray(coef, np.float64).reshape(27).tobytes()
    buf = L.GPU_MakeBuffer(len(raw), pbrhip.BufferFlag_CPU if host else pbrhip.BufferFlag_GPU, raw)
    assert buf
    return buf


def write_coef(buf, coef):
    raw = np.ascontiguousarray(coef, np.float64).reshape(27).tobytes()
    C.memmove(buf.contents.data, raw, 216)


def draw_sh(rig, flags, buf, offset=0, rows=None, graph=None):
    """The rig's pass recorded in SH mode (flags: without the SH9 bit) from `buf`, submitted and waited for -> the target"""
    L = rig.L
    pipe = L.PBR_LightingPipeline(rig.lp)
    L.GPUX_SetShadeFlags(pipe, flags | SH9)
    L.GPUX_SetShadeSH9(pipe, buf, offset)
    g = rig.g if graph is None else graph
    r0, r1 = rows or (0, 0)
    L.PBR_RecordLightingPass(rig.lp, g, C.byref(rig.case.glob), r0, r1)
    L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
    return rig.read()


def check(case, comp, coef, got, label, rows=None):
    """got against max(F0 + d E, 0) inside `rows` (default: the frame), on the screened pixels -> largest error"""
    import pbr_oracle as O
    want = comp.want(coef)
    y0, y1 = rows or (0, case.H)
    sel = np.zeros((case.H, case.W), bool)
    sel[y0:y1] = True
    sel &= comp.keep
    assert comp.share <= SM.SCREEN_CAP and comp.keep[~case.surface].all()
    if got.dtype == np.float16:
        gb = got.view(np.uint16).astype(np.int32)
        wb = O.f32_to_f16_bits(want.astype(np.float32)).astype(np.int32)
        d = np.abs(gb[..., :3] - wb[..., :3]).max(-1)
        e = int(d[sel].max())
        print(f"{label}: fp16 codes off {e}")
        assert e <= 1, (label, e, np.argwhere(sel & (d > 1))[:5].tolist())
        assert (gb[y0:y1, :, 3] == 0x3C00).all(), label
        return e
    assert not np.isnan(got).any(), label
    m = SM.rel_map(got, want)
    e = float(m[sel].max())
    print(f"{label}: rel_err {e:.3e}, screen removed {100 * comp.share:.3f} % of {int(case.surface.sum())} surface pixels")
    assert e < SM.REL, (label, e, np.argwhere(sel & (m >= SM.REL))[:5].tolist())
    assert (got[y0:y1, :, 3] == 1.0).all(), label
    return e


FRAMES = [(s, "f32") for s in SM.RAGGED] + [((65, 5), "f16")]


@pytest.mark.parametrize("size,fmt", FRAMES, ids=[f"{s[0]}x{s[1]}-{f}" for s, f in FRAMES])
def test_sh_frame_against_the_composite_reference(gpu, size, fmt):
    """IBL | SH9 and IBL | SHAFTS | SH9 (k_shade_fast<.., .., true>), IBL | SHADOWS | SH9 (k_shade<false, true>) with a set of coefficients
    whose irradiance is positive everywhere and one whose irradiance is negative over part of the sphere: where F0 + d E < 0 the
    shader's final clamp gives exactly 0.  The wild normals are as short as 0.007 and as long as 1.7: the SH form is evaluated for N
    as it is."""
    case, _ = reference(size, IBL)
    rig = ShadeRig(gpu, case, _fmt(fmt))
    sets = {"positive": SR.coef_positive(), "partly negative": SR.coef_partly_negative()}
    bufs = {k: coef_buffer(gpu, c) for k, c in sets.items()}
    clamped_seen = 0
    try:
        for flags, kernel in FLAG_SETS:
            _, comp = reference(size, flags)
            for name, coef in sets.items():
                got = draw_sh(rig, flags, bufs[name])
                assert gpu.pbrk_shade_last_kernel() == kernel, (flags, name)
                check(case, comp, coef, got, f"sh9 {size[0]}x{size[1]} {fmt} flags {flags} {name}")
                if name == "partly negative":
                    deep = (comp.F0[..., :3].astype(np.float64) + comp.d * SR.irradiance_at(coef, comp.N)) < -1e-3
                    assert (got[..., :3][deep] == 0).all()
                    clamped_seen += int(deep.any(-1).sum())
                else:
                    assert not comp.clamped(coef).any()
        if size == (130, 9):
            assert clamped_seen >= 10, clamped_seen                          # the clamp acted (test_sh_shade_cpu.py counts per flag set)
            length = np.linalg.norm(comp.N, axis=-1)[case.surface & comp.keep]
            assert length.min() < 0.1 and length.max() > 1.5, (length.min(), length.max())
    finally:
        rig.destroy()
        for b in bufs.values():
            gpu.GPU_DestroyBuffer(b)


@pytest.mark.parametrize("flags,kernel", [(IBL, FAST), (IBL | SHADOWS, GENERAL)], ids=["fast", "general"])
def test_row_band_through_draw_rows(gpu, flags, kernel):
    """GPUX_OpDrawRows(2, 7) of the 130 x 9 frame: the band equals the reference and the whole-frame draw bit for bit, the rows outside
    keep their clear value"""
    size, rows = (130, 9), (2, 7)
    case, comp = reference(size, flags)
    rig = ShadeRig(gpu, case)
    coef = SR.coef_partly_negative()
    buf = coef_buffer(gpu, coef)
    try:
        whole = draw_sh(rig, flags, buf)
        rig.clear()
        got = draw_sh(rig, flags, buf, rows=rows)
        assert gpu.pbrk_shade_last_kernel() == kernel
        assert (got[:rows[0]] == -7.0).all() and (got[rows[1]:] == -7.0).all()
        assert np.array_equal(got[rows[0]:rows[1]].view(np.uint32), whole[rows[0]:rows[1]].view(np.uint32))
        check(case, comp, coef, got, f"sh9 rows {rows} flags {flags}", rows=rows)
    finally:
        rig.destroy()
        gpu.GPU_DestroyBuffer(buf)


def test_gi_frame_without_an_irradiance_binding_equals_the_bound_one(gpu):
    """IBL | GI | SH9: the trace overwrites `ambient`, so the flag only lifts the need for TEX_IRRADIANCE_MAP.  A pass made from maps
    without an irradiance cube, and pbrk_shade with irradiance_bordered == NULL, give the bits of IBL | GI with the cube bound."""
    import pbrhip
    L = gpu
    W, H = SM.RAGGED_GI[0]
    case = SM.ShadeCase(W, H, 64, 32, 64, gi=True)
    rig = ShadeRig(L, case)
    buf = coef_buffer(L, SR.coef_positive())
    bare = pbrhip.PBR_IBLMaps()
    bare.brdf_lut, bare.tex_specular_env_map = rig.maps.brdf_lut, rig.maps.tex_specular_env_map          # irradiance_map stays NULL
    lp = L.PBR_MakeLightingPassLive(C.byref(rig.gb), C.byref(bare), W, H, rig.sun_tex, rig.grid_tex, rig.prev_tex)
    assert lp
    try:
        bound = rig.draw_api(IBL | GI)
        assert L.pbrk_shade_last_kernel() == LIVE
        rig.clear()
        L.GPUX_SetShadeFlags(L.PBR_LightingPipeline(lp), IBL | GI)
        L.PBR_LightingUseSH9(lp, buf, 0)
        assert L.GPUX_GetShadeFlags(L.PBR_LightingPipeline(lp)) == IBL | GI | SH9
        L.PBR_RecordLightingPass(lp, rig.g, C.byref(case.glob), 0, 0)
        L.GPU_GraphSubmit(rig.g); L.GPU_GraphWait(rig.g)
        assert L.pbrk_shade_last_kernel() == LIVE
        assert np.array_equal(rig.read().view(np.uint32), bound.view(np.uint32))
        tw = rig.build_twins()
        rig.clear()
        a = rig.args(IBL | GI | SH9, tw)
        a.irradiance_bordered, a.irradiance_cells, a.irradiance_size = None, None, 0
        a.sh9_coef = L.GPUX_BufferDevicePtr(buf)
        assert rig.shade_abi(a) == 0 and L.pbrk_shade_last_kernel() == LIVE
        assert np.array_equal(rig.read().view(np.uint32), bound.view(np.uint32))
    finally:
        L.GPU_WaitUntilIdle()
        L.PBR_DestroyLightingPass(lp)
        rig.destroy()
        L.GPU_DestroyBuffer(buf)


def test_coefficients_produced_on_the_device(gpu):
    """GPUX_OpProjectSH9 of a 16^2 cube level and the shade in one graph, and the projection in graph A with the shade in graph B
    submitted back to back: both frames have the bits of the frame shaded from the same 27 numbers uploaded from the host, which is
    the reference's frame for them."""
    import pbrhip
    L = gpu
    size, flags = (65, 5), IBL
    case, comp = reference(size, flags)
    rig = ShadeRig(L, case)
    env = SM.cube_level(16, 0, variant=2)
    tex = pbrhip.make_texture(pbrhip.Format_RGBA32F, 16, 16, pbrhip.TextureFlag_Cubemap, env)
    coef = pbrhip.project_sh9(tex, 0)
    want, S = R.project(env)
    assert R.worst_ratio(np.abs(coef - want), S) <= 1e-10
    bufs = [coef_buffer(L, coef)] + [coef_buffer(L, np.zeros(27)) for _ in range(2)]
    graph_a = L.GPU_MakeGraph()
    try:
        from_host = draw_sh(rig, flags, bufs[0])
        assert L.pbrk_shade_last_kernel() == FAST
        check(case, comp, coef, from_host, "sh9 coefficients of a 16^2 level, uploaded")
        rig.clear()
        L.GPUX_OpProjectSH9(rig.g, tex, 0, 0, 6, 0, 16, bufs[1], 0)
        one_graph = draw_sh(rig, flags, bufs[1])
        assert np.array_equal(one_graph.view(np.uint32), from_host.view(np.uint32))
        rig.clear()
        L.GPUX_OpProjectSH9(graph_a, tex, 0, 0, 6, 0, 16, bufs[2], 0)
        L.GPU_GraphSubmit(graph_a)                                           # no wait: graph B follows it on the device
        two_graphs = draw_sh(rig, flags, bufs[2])
        L.GPU_GraphWait(graph_a)
        assert np.array_equal(two_graphs.view(np.uint32), from_host.view(np.uint32))
    finally:
        L.GPU_WaitUntilIdle()
        L.GPU_DestroyGraph(graph_a)
        rig.destroy()
        L.GPU_DestroyTexture(tex)
        for b in bufs:
            L.GPU_DestroyBuffer(b)


def test_replayed_graph_sees_new_coefficients(gpu):
    """Under GPUX_SetGraphReplay(1) the same graph is submitted twice with other numbers in the same (mapped) buffer: each frame is the
    reference's for the numbers the buffer held when it ran, and has the bits of a plain submission."""
    L = gpu
    size, flags = (65, 5), IBL | SHAFTS
    case, comp = reference(size, flags)
    rig = ShadeRig(L, case)
    sets = (SR.coef_positive(), SR.coef_partly_negative())
    buf = coef_buffer(L, sets[0], host=True)
    g = L.GPU_MakeGraph()
    try:
        plain = []
        for coef in sets:                                                    # also builds the twins: the graph below is replayable
            write_coef(buf, coef)
            plain.append(draw_sh(rig, flags, buf))
        L.GPUX_SetGraphReplay(1)
        for coef, want_bits in zip(sets, plain):
            write_coef(buf, coef)
            rig.clear()
            got = draw_sh(rig, flags, buf, graph=g)
            check(case, comp, coef, got, "sh9 under replay")
            assert np.array_equal(got.view(np.uint32), want_bits.view(np.uint32))
        s = [C.c_uint64() for _ in range(3)]
        L.GPUX_GraphReplayStats(g, *[C.byref(v) for v in s])
        print(f"replay: launches {s[0].value}, updates {s[1].value}, instantiations {s[2].value}")
        assert s[0].value == 2
        assert not np.array_equal(plain[0], plain[1])
    finally:
        L.GPUX_SetGraphReplay(-1)
        L.GPU_WaitUntilIdle()
        L.GPU_DestroyGraph(g)
        rig.destroy()
        L.GPU_DestroyBuffer(buf)


def _timed_names(L, g):
    return [L.GPUX_GraphTimedOpName(g, i).decode() for i in range(L.GPUX_GraphTimedOpCount(g))]


def test_no_irradiance_twin_is_built(gpu):
    """A fresh pass with TEX_IRRADIANCE_MAP bound, drawn in SH mode: the timed ops of its first graph build the prefiltered cube's twins
    and run K5, and hold no apron.irradiance; the cube path's first graph on the same pass then does build it."""
    L = gpu
    case, comp = reference((63, 3), IBL)
    rig = ShadeRig(L, case)
    coef = SR.coef_positive()
    buf = coef_buffer(L, coef)
    L.GPUX_EnableOpTiming(1)
    try:
        got = draw_sh(rig, IBL, buf)
        names = _timed_names(L, rig.g)
        print("sh9 first graph:", names)
        assert "K5.shade" in names and "apron.prefiltered" in names and "apron.irradiance" not in names
        check(case, comp, coef, got, "sh9 first frame of a fresh pass")
        rig.draw_api(IBL)
        names = _timed_names(L, rig.g)
        print("cube path first graph:", names)
        assert "apron.irradiance" in names and "apron.prefiltered" not in names
    finally:
        L.GPUX_EnableOpTiming(0)
        rig.destroy()
        L.GPU_DestroyBuffer(buf)


class _Errors:
    def __init__(self, L):
        self.L, self.msgs = L, []
        self.cb = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)(lambda m, u: self.msgs.append(m.decode()))

    def __enter__(self):
        self.L.GPUX_SetErrorHandler(C.cast(self.cb, C.c_void_p), None)
        return self

    def __exit__(self, *a):
        self.L.GPUX_SetErrorHandler(None, None)


def test_record_time_checks(gpu):
    """The flag without a buffer, without GPUX_Shade_IBL, with an offset that is no multiple of 8 and with fewer than 216 bytes behind the
    offset: one message each, nothing recorded, the cleared target stays as it is; the same buffer at a good offset is accepted."""
    L = gpu
    case, comp = reference((63, 3), IBL)
    rig = ShadeRig(L, case)
    coef = SR.coef_positive()
    buf = coef_buffer(L, coef, pad=216)                                      # 432 bytes, the numbers at 216
    pipe = L.PBR_LightingPipeline(rig.lp)
    try:
        rig.clear()
        with _Errors(L) as e:
            for flags, b, off, needle in ((IBL | SH9, None, 0, "without a coefficient buffer"), (SH9, buf, 216, "needs GPUX_Shade_IBL"),
                                          (SHAFTS | SH9, buf, 216, "needs GPUX_Shade_IBL"), (IBL | SH9, buf, 4, "multiple of 8"),
                                          (IBL | SH9, buf, 220, "multiple of 8"), (IBL | SH9, buf, 224, "too small"), (IBL | SH9, buf, 432, "too small")):
                e.msgs.clear()
                L.GPUX_SetShadeFlags(pipe, flags)
                L.GPUX_SetShadeSH9(pipe, b, off)
                L.PBR_RecordLightingPass(rig.lp, rig.g, C.byref(case.glob), 0, 0)
                assert len(e.msgs) == 1 and needle in e.msgs[0], (flags, off, e.msgs)
                e.msgs.clear()
                L.GPU_GraphSubmit(rig.g); L.GPU_GraphWait(rig.g)
                assert e.msgs == [] and (rig.read() == -7.0).all(), (flags, off, e.msgs)
            e.msgs.clear()
            got = draw_sh(rig, IBL, buf, offset=216)
            assert e.msgs == []
        check(case, comp, coef, got, "sh9 coefficients at offset 216")
    finally:
        rig.destroy()
        L.GPU_DestroyBuffer(buf)


def test_kernel_abi_checks(gpu):
    """pbrk_shade with PBRK_SHADE_SH9: a NULL or misaligned sh9_coef is refused and nothing is launched; without PBRK_SHADE_IBL the flag
    means nothing; with it the irradiance arguments may all be NULL"""
    L = gpu
    case, comp = reference((63, 3), IBL)
    rig = ShadeRig(L, case)
    coef = SR.coef_positive()
    buf = coef_buffer(L, coef)
    try:
        tw = rig.build_twins()
        rig.clear()
        for ptr in (None, L.GPUX_BufferDevicePtr(buf) + 4):
            a = rig.args(IBL | SH9, tw)
            a.sh9_coef = ptr
            assert rig.shade_abi(a) == E_ARG
        assert (rig.read() == -7.0).all()
        a = rig.args(SH9, tw)
        assert rig.shade_abi(a) == 0
        plain = rig.read()
        assert rig.shade_abi(rig.args(0, tw)) == 0
        assert np.array_equal(plain.view(np.uint32), rig.read().view(np.uint32))
        a = rig.args(IBL | SH9, tw)
        a.irradiance_bordered, a.irradiance_cells, a.irradiance_size = None, None, 0
        a.sh9_coef = L.GPUX_BufferDevicePtr(buf)
        assert rig.shade_abi(a) == 0 and L.pbrk_shade_last_kernel() == FAST
        check(case, comp, coef, rig.read(), "sh9 through the kernel ABI, no irradiance arguments")
    finally:
        rig.destroy()
        L.GPU_DestroyBuffer(buf)


def test_switching_off_returns_to_the_cube_path(gpu):
    """PBR_LightingUseSH9(lp, buf, 0) sets flag and buffer, (lp, NULL, 0) clears them: the frame after equals the frame before SH mode
    bit for bit, and the frame in between is another one"""
    L = gpu
    case, comp = reference((65, 5), IBL)
    rig = ShadeRig(L, case)
    coef = SR.coef_positive()
    buf = coef_buffer(L, coef)
    pipe = L.PBR_LightingPipeline(rig.lp)

    def draw():
        L.PBR_RecordLightingPass(rig.lp, rig.g, C.byref(case.glob), 0, 0)
        L.GPU_GraphSubmit(rig.g); L.GPU_GraphWait(rig.g)
        return rig.read()

    try:
        L.GPUX_SetShadeFlags(pipe, IBL | SHAFTS)
        before = draw()
        L.PBR_LightingUseSH9(rig.lp, buf, 0)
        assert L.GPUX_GetShadeFlags(pipe) == IBL | SHAFTS | SH9
        during = draw()
        _, comp_shafts = reference((65, 5), IBL | SHAFTS)
        check(case, comp_shafts, coef, during, "sh9 through PBR_LightingUseSH9")
        L.PBR_LightingUseSH9(rig.lp, None, 0)
        assert L.GPUX_GetShadeFlags(pipe) == IBL | SHAFTS
        after = draw()
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        assert not np.array_equal(before, during)
    finally:
        rig.destroy()
        L.GPU_DestroyBuffer(buf)


def test_demo_sh9shade_option(gpu, tmp_path):
    """pbr_demo ... sh9shade: one more line, frame_sh9_checksum; every other line is what the demo prints without the option"""
    import subprocess
    import pbrhip
    from pbrhip import synth
    hdr = tmp_path / "cube_strip.hdr"
    hdr.write_bytes(synth.env_to_hdr_strip(synth.synth_env(32, seed=0x5EED0017), rle=True))
    exe = os.path.join(pbrhip.PKG_ROOT, "pbr_demo")
    sizes = ["16", "64", "32", "16", "96", "54"]

    def lines(extra):
        out = subprocess.run([exe, str(hdr), *sizes, *extra], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return [l for l in out.stdout.splitlines() if not l.startswith("time_ms")]

    plain, with_sh = lines([]), lines(["sh9shade"])
    extra = [l for l in with_sh if l.startswith("frame_sh9_checksum")]
    assert len(extra) == 1 and np.isfinite(float(extra[0].split()[1])) and float(extra[0].split()[1]) > 0
    assert [l for l in with_sh if not l.startswith("frame_sh9_checksum")] == plain and plain[-1] == "ok 1"
    # (the demo's floor is fully metallic, kD == 0: its frame does not say which ambient term it had; the tests above do)
