"""Independent whole levels of one submission side by side on side streams (GPU_GraphSubmit, TileRegion: GPUX_SetLevelOverlap,
GPUX_LevelOverlapCount) against the serial chain: the bytes of every level must not depend on it, dispatches that depend on each
other must stay in order, and the counter must show which path a submission took.  No case compares times.

One small job: a 256^2 environment, a 512^2 specular cube (10 levels) and a 32^2 irradiance map.  Level 1 (256^2 outputs from the
16^2 source level) is the smallest the region kernel accepts, levels 2 to 9 run on the level-in-LDS kernel, level 0 is the copy:
about 2e9 sample evaluations, a few milliseconds."""
import ctypes as C

import numpy as np
import pytest

import pbrhip
from pbrhip import mc

pytestmark = pytest.mark.gpu

W, S, IRR = 256, 512, 32


def _unit(kind, mip, size):
    return pbrhip.PBR_WorkUnit(kind, mip, 0, 6, 0, size, 0.0)


def _whole_job(spec, irr, env):
    arr, n = pbrhip.partition(spec, 1, irr, env, 1, 0)
    return [arr[i] for i in range(n)]


def _digests(maps):
    n = maps.tex_specular_env_map.contents.mip_level_count
    return [mc.digest(pbrhip.read_mip(maps.tex_specular_env_map, m)) for m in range(n)] + [mc.digest(pbrhip.read_mip(maps.irradiance_map, 0))]


class Rig:
    """Maps, pipelines, an arena and a graph for submissions of work units; `submit` returns what the submission reported."""

    def __init__(self, L, irr=IRR, spec=S):
        self.L = L
        self.maps = pbrhip.PBR_IBLMaps()
        L.PBR_MakeIBLMaps(C.byref(self.maps), irr, 64, spec)
        self.pipes = L.PBR_MakeIBLPipelines(); self.arena = L.GPU_MakeDescriptorArena(); self.g = L.GPU_MakeGraph()

    def record(self, env_tex, units, maps=None):
        arr = (pbrhip.PBR_WorkUnit * len(units))(*units)
        self.L.PBR_RecordUnits(self.pipes, self.g, self.arena, env_tex, C.byref(maps or self.maps), arr, len(units))

    def submit(self):
        """-> (GPUX_LevelOverlapCount, the timed-op names in the order they are reported) of the submission, waited for."""
        L = self.L
        L.GPU_GraphSubmit(self.g)
        count = L.GPUX_LevelOverlapCount()
        L.GPU_GraphWait(self.g); L.GPU_ResetDescriptorArena(self.arena)
        return count, [L.GPUX_GraphTimedOpName(self.g, i).decode() for i in range(L.GPUX_GraphTimedOpCount(self.g))]

    def free(self):
        L = self.L
        L.GPU_DestroyGraph(self.g); L.GPU_DestroyDescriptorArena(self.arena); L.PBR_DestroyIBLPipelines(self.pipes)
        L.PBR_DestroyIBLMaps(C.byref(self.maps))


def _run_units(L, env_tex, units, regenerate=False):
    """The job through PBR_RecordUnits in one submission -> (level digests, count, timed-op names)."""
    rig = Rig(L)
    try:
        if regenerate:
            L.GPU_OpGenerateMipmaps(rig.g, env_tex)
        rig.record(env_tex, units)
        count, names = rig.submit()
        return _digests(rig.maps), count, names
    finally:
        rig.free()


def _run_plain(L, env_tex):
    """The job through GPU_OpDispatch of whole levels: the reference's two calls -> (level digests, count of each call)."""
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), IRR, 64, S)
    try:
        L.PBR_GenPrefilteredEnvMap(env_tex, maps.tex_specular_env_map, 1)
        c_spec = L.GPUX_LevelOverlapCount()
        L.PBR_GenIrradianceMap(env_tex, maps.irradiance_map)
        c_irr = L.GPUX_LevelOverlapCount()
        return _digests(maps), c_spec, c_irr
    finally:
        L.PBR_DestroyIBLMaps(C.byref(maps))


@pytest.fixture(scope="module")
def job(gpu):
    """(environment texture, the job's units, the serial chain's level digests and its timed-op names in order).  Per-op timing is on for the
    module; the settings go back to their defaults after it."""
    L = gpu
    env = np.random.default_rng(0x1E7E1).random((6, W, W, 4), dtype=np.float32) + 0.1
    tex = mc.env_texture(env)
    units = _whole_job(S, IRR, W)
    L.GPUX_EnableOpTiming(1)
    try:
        L.GPUX_SetLevelOverlap(0)
        mc.reset_counters(L)
        first, _, first_names = _run_units(L, tex, units)                     # builds the environment's apron and cells
        serial, count, names = _run_units(L, tex, units)
        st = mc.counters(L, "region", reset=True)
        L.GPUX_SetLevelOverlap(1)
        assert count == 0 and first == serial and set(first_names) == set(names) | {"apron.env", "cells.env"}, (first_names, names)
        assert st["slices"] > 0 and st["healed"] == 0, st                       # the region kernel ran: level 1
        assert {"K4a.prefilter_copy.mip0", "K3.irradiance"} | {f"K4b.prefilter_mc.mip{m}" for m in range(1, 10)} <= set(names), names
        yield tex, units, serial, names
    finally:
        L.GPUX_SetLevelOverlap(1); L.GPUX_SetTileStreams(-1); L.GPUX_EnableOpTiming(0)
        L.GPU_DestroyTexture(tex)


def test_same_bytes_both_recording_forms(gpu, job):
    L = gpu
    tex, units, serial, serial_names = job
    try:
        mc.reset_counters(L)
        on, count, names = _run_units(L, tex, units)
        st = mc.counters(L, "region", reset=True)
        assert on == serial
        assert count == len(units) >= 2, count
        assert names == serial_names, (names, serial_names)            # the same ops, reported in recording order
        assert st["slices"] > 0 and st["healed"] == 0, st
        plain_on, c_spec, c_irr = _run_plain(L, tex)
        assert plain_on == serial
        assert c_spec == len(units) - 1 and c_irr == 0, (c_spec, c_irr)           # ten levels in one graph; the irradiance map alone in its own

        L.GPUX_SetLevelOverlap(0)
        plain_off, c_spec, c_irr = _run_plain(L, tex)
        assert plain_off == serial and c_spec == 0 and c_irr == 0, (c_spec, c_irr)
        L.GPUX_SetLevelOverlap(1)

        L.GPUX_SetTileStreams(1)
        one, count, names = _run_units(L, tex, units)
        assert one == serial and count == 0 and names == serial_names, (count, names)
        plain_one, c_spec, c_irr = _run_plain(L, tex)
        assert plain_one == serial and c_spec == 0 and c_irr == 0, (c_spec, c_irr)
    finally:
        L.GPUX_SetLevelOverlap(1); L.GPUX_SetTileStreams(-1)


@pytest.mark.parametrize("streams", [2, 3, 4])
def test_same_bytes_on_every_stream_count(gpu, job, streams):
    L = gpu
    tex, units, serial, _ = job
    try:
        L.GPUX_SetLevelStreams(streams)
        on, count, _ = _run_units(L, tex, units)
        assert on == serial and count == len(units)
    finally:
        L.GPUX_SetLevelStreams(-1)


def _chain(L, tex, first, between, second, together):
    """Units `first` prefilter the environment into cube B; `between` (irradiance units) and `second` (prefilter units) sample B.  In
    one submission (`together`) or in two -> (digests of what sampled B, count of the one submission or of the second)."""
    b = Rig(L, irr=16, spec=64)
    c = Rig(L, irr=16, spec=32)
    try:
        b.record(tex, first)
        if not together:
            b.submit()
        b.record(b.maps.tex_specular_env_map, between + second, maps=c.maps)
        count, _ = b.submit()
        return _digests(c.maps), count
    finally:
        c.free(); b.free()


@pytest.mark.parametrize("with_irradiance", [False, True])
def test_a_dispatch_that_samples_what_the_submission_writes_stays_behind_it(gpu, job, with_irradiance):
    L = gpu
    tex = job[0]
    first = _whole_job(64, 16, W)                                   # 7 levels of B and an irradiance map, all from the environment
    between = [_unit(pbrhip.Unit_Irradiance, 0, 16)] if with_irradiance else []
    second = [u for u in _whole_job(32, 0, 64)]                     # 6 levels of C from B
    one, count = _chain(L, tex, first, between, second, together=True)
    two, count2 = _chain(L, tex, first, between, second, together=False)
    assert one == two
    assert count == len(first) + len(between) + len(second) and count2 == len(between) + len(second), (count, count2)
    # The count tells the regions apart where one side of the hazard is a single dispatch: it runs alone, outside any region
    if not with_irradiance:
        lone = [_unit(pbrhip.Unit_Prefilter, 1, 16)]
        one, count = _chain(L, tex, first, [], lone, together=True)
        two, _ = _chain(L, tex, first, [], lone, together=False)
        assert one == two and count == len(first), count              # had the reader of B joined B's writers: len(first) + 1
    else:
        lone = [_unit(pbrhip.Unit_Prefilter, 4, 4)]                   # the level of B that level 1 of C samples; then B's irradiance and two levels of C
        pair = [_unit(pbrhip.Unit_Prefilter, 1, 16), _unit(pbrhip.Unit_Prefilter, 2, 8)]
        one, count = _chain(L, tex, lone, between, pair, together=True)
        two, _ = _chain(L, tex, lone, between, pair, together=False)
        assert one == two and count == 3, count                       # 4: the irradiance map joined the writer of B; 2: it was left alone


def test_twins_rebuilt_inside_the_submission(gpu, job):
    """New content in level 0 of the environment: the submission regenerates the mip chain and rebuilds apron and cells."""
    L = gpu
    _, units, serial, serial_names = job
    env2 = np.random.default_rng(0x1E7E2).random((6, W, W, 4), dtype=np.float32) + 0.1
    tex = mc.env_texture(np.zeros_like(env2))
    try:
        results = []
        for on in (0, 1):
            L.GPUX_SetLevelOverlap(on)
            pbrhip.upload_mip(tex, 0, env2)
            results.append(_run_units(L, tex, units, regenerate=True))
        (off_levels, off_count, off_names), (on_levels, on_count, on_names) = results
        assert on_levels == off_levels and on_levels != serial
        assert off_count == 0 and on_count == len(units)
        assert on_names == off_names and set(on_names) == set(serial_names) | {"apron.env", "cells.env", "K2.mip_chain"}, (on_names, off_names)
    finally:
        L.GPUX_SetLevelOverlap(1)
        L.GPU_DestroyTexture(tex)


def test_a_job_of_one_dispatch_opens_no_region(gpu, job):
    L = gpu
    tex, units, serial, _ = job
    rig = Rig(L)
    try:
        rig.record(tex, [units[2]])
        count, names = rig.submit()
        assert count == 0 and names == ["K4b.prefilter_mc.mip2"], (count, names)
        assert mc.digest(pbrhip.read_mip(rig.maps.tex_specular_env_map, 2)) == serial[2]
    finally:
        rig.free()


def test_sharded_units_equal_the_whole_job(gpu, job):
    """Each rank's units of a three-way partition submitted on this GPU, overlap on."""
    L = gpu
    tex, units, serial, _ = job
    rig = Rig(L)
    try:
        for rank in range(3):
            arr, n = pbrhip.partition(S, 1, IRR, W, 3, rank)
            rig.record(tex, [arr[i] for i in range(n)])
            rig.submit()
        assert _digests(rig.maps) == serial
    finally:
        rig.free()
