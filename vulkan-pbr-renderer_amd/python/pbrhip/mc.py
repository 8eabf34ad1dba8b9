"""Harness of the K4b region kernel (k_mc_region.hip) for the tests and the probes under tools/: its switches, its counters
by name, device buffers, bordered levels, prefilter tables, and the two ways it is driven (row windows through pbrk_mc_filter,
work units through PBR_RecordUnits).  Importing this loads no library and touches no GPU; every function takes the loaded
library `L` (pbrhip.lib() / pbrhip.init())."""
import contextlib
import ctypes as C
import hashlib

import numpy as np

import pbrhip

# switch -> the library's default: pbrk_mc_set_<switch>(*default)
SWITCH_DEFAULTS = {"absorb": (1,), "runs": (1,), "prologue": (1,), "launch_cut": (1,), "tile32": (-1,), "fold": (1,), "net": (-1,),
                   "kernels": (-1, -1), "bin_cache": (-1,), "exact_bins": (-1,)}


@contextlib.contextmanager
def switches(L, **named):
    """Set the named switches (absorb, runs, prologue, launch_cut, tile32, fold, net, bin_cache, exact_bins, kernels=(lds, region)) for the body and no others.
    On exit, also on an exception, exactly those go back to the library's DEFAULTS, not to their previous values: the library
    has no getters."""
    unknown = set(named) - set(SWITCH_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown switch {sorted(unknown)}: one of {sorted(SWITCH_DEFAULTS)}")
    for name, value in named.items():
        getattr(L, "pbrk_mc_set_" + name)(*(value if name == "kernels" else (value,)))
    try:
        yield
    finally:
        for name in named:
            getattr(L, "pbrk_mc_set_" + name)(*SWITCH_DEFAULTS[name])


# group -> (getter, slot type, slots, how the slots become keys)
_GROUPS = {
    "region": ("pbrk_mc_region_stats", C.c_uint64, 2, lambda a: {"healed": int(a[0]), "slices": int(a[1])}),
    "skip": ("pbrk_mc_region_skip_stats", C.c_uint64, 3, lambda a: {"abs_words": int(a[0]), "abs_samples": int(a[1]), "count_only": int(a[2])}),
    "flag": ("pbrk_mc_region_flag_stats", C.c_uint64, 3, lambda a: {"flags": int(a[0]), "flag_samples": int(a[1]), "visits": int(a[2])}),
    "window": ("pbrk_mc_region_window_stats", C.c_uint64, 1, lambda a: {"proved": int(a[0])}),
    "cut": ("pbrk_mc_launch_cut_stats", C.c_int, 6, lambda a: {"cut4": list(a)[:4], "nw": int(a[4]), "words_cut": int(a[5])}),
    "phase": ("pbrk_mc_region_phase_stats", C.c_uint64, 5, lambda a: {"phase": tuple(int(v) for v in a)}),
}


def counters(L, *groups, reset=False, missing_ok=False):
    """The counters of the named groups in one dict ("cut": of the last launch).  Only their getters are called, "region" (healed,
    slices) last whatever the order of `groups`: `reset` goes to that call alone, and pbrk_mc_region_stats(buf, 1) zeroes every
    group.  A getter that fails (no launch yet, PBR_MC_STATS off) raises AssertionError, or with `missing_ok` leaves its keys out."""
    out = {}
    for group in sorted(groups, key=lambda g: g == "region"):
        getter, ctype, n, keys = _GROUPS[group]
        buf = (ctype * n)()
        rc = getattr(L, getter)(buf, int(reset)) if group == "region" else getattr(L, getter)(buf)
        assert rc == 0 or missing_ok, f"{getter} returned {rc}"
        if rc == 0:
            out.update(keys(buf))
    return out


BIN_CACHE_KEYS = ("recorded", "replayed", "computed", "declined", "bytes")


def bin_cache_stats(L):
    """pbrk_mc_bin_cache_stats by name: launches that recorded / replayed / computed though the cache was on / were declined for the
    budget since the library was loaded, and the bytes held now."""
    buf = (C.c_uint64 * 5)()
    L.pbrk_mc_bin_cache_stats(buf)
    return dict(zip(BIN_CACHE_KEYS, (int(v) for v in buf)))


EXACT_BINS_KEYS = ("flags_before", "flags_after", "proved_before", "proved_after", "any_before", "any_after", "unset_hits", "lost_lanes")


def exact_bins_stats(L, reset=False):
    """pbrk_mc_exact_bins_stats by name, summed over the entries refined since the last reset; unset_hits and lost_lanes must be 0."""
    buf = (C.c_uint64 * 8)()
    assert L.pbrk_mc_exact_bins_stats(buf, int(reset)) == 0
    return dict(zip(EXACT_BINS_KEYS, (int(v) for v in buf)))


PLAN_FIELDS = ("family", "RS", "G", "RC", "NR", "NW", "tile", "nslices", "runs", "lean", "fold", "net", "absorb", "head_first", "prep", "cut",
               "stats", "bin_cache", "bin_eligible", "whole", "refine", "bin_flavour", "lds", "lds_slices", "direct_slices")
PLAN_FAMILIES = ("declined", "region", "resident")


class PbrkMcPlan(C.Structure):
    _fields_ = [(name, C.c_int) for name in PLAN_FIELDS] + [("expect", C.c_int * 16)]


def _targs(*values):
    return "<" + ", ".join(str(v).lower() if isinstance(v, bool) else str(v) for v in values) + ">"


def plan(L, n_src, n_tab, size, window=None, counters=False, have_prep=True):
    """pbrk_mc_plan by name, for the library's switches as they stand: what one pbrk_mc_filter dispatch of the window (face0, face1, y0,
    rows; default: the whole level) would decide.  Touches no GPU.  Besides the struct's fields: "family" by name, "kernel" -- the region,
    resident, level-in-LDS or direct instantiation (without cells, sampler snap off) as a demangled kernel name spells it --, and
    "refine_kernel", the k_mc_refine_bins instantiation that follows the launch IF it records (plan["refine"])."""
    f0, f1, y0, rows = window or (0, 6, 0, size)
    raw = PbrkMcPlan()
    rc = L.pbrk_mc_plan(n_src, n_tab, size, f0, f1 - f0, y0, rows, int(counters), int(have_prep), C.byref(raw))
    assert rc == 0, f"pbrk_mc_plan returned {rc}"
    p = {name: getattr(raw, name) for name in PLAN_FIELDS}
    p["expect"] = list(raw.expect)
    p["family"] = PLAN_FAMILIES[raw.family]
    sub = raw.tile == 32 or raw.G > 1
    p["refine_kernel"] = None
    p["kernel"] = "k_mc_filter_lds" + _targs(raw.lds_slices) if raw.lds_slices else "k_mc_filter" + _targs(raw.direct_slices, 4, False, False)
    if p["family"] == "region":
        p["kernel"] = "k_mc_region" + _targs(raw.RS, sub, raw.tile, bool(raw.runs), bool(raw.lean), bool(raw.fold), bool(raw.net))
        p["refine_kernel"] = "k_mc_refine_bins" + _targs(raw.RS, sub, raw.tile, bool(raw.fold))
    elif p["family"] == "resident":
        p["kernel"] = "k_mc_resident" + _targs(raw.tile, bool(raw.fold), bool(raw.stats))
    return p


def reset_counters(L):
    """Zero every counter.  The return code is ignored: the counters exist only after the kernel's first launch."""
    L.pbrk_mc_region_stats((C.c_uint64 * 2)(), 1)


class DeviceBuffer:
    """A device buffer of the backend (GPU_MakeBuffer), optionally filled from a numpy array."""

    def __init__(self, L, nbytes, data=None):
        self.L, self.nbytes = L, nbytes
        self.buf = L.GPU_MakeBuffer(nbytes, pbrhip.BufferFlag_GPU, data.ctypes.data_as(C.c_void_p) if data is not None else None)
        assert self.buf
        self.ptr = L.GPUX_BufferDevicePtr(self.buf)

    def read(self):
        L = self.L
        host = L.GPU_MakeBuffer(self.nbytes, pbrhip.BufferFlag_CPU, None)
        g = L.GPU_MakeGraph()
        try:
            L.GPU_WaitUntilIdle()
            L.GPU_OpCopyBufferToBuffer(g, self.buf, host, 0, 0, self.nbytes); L.GPU_GraphSubmit(g); L.GPU_GraphWait(g)
            return bytes((C.c_char * self.nbytes).from_address(host.contents.data))
        finally:
            L.GPU_DestroyGraph(g)
            L.GPU_DestroyBuffer(host)

    def free(self):
        if self.buf:
            self.L.GPU_WaitUntilIdle()
            self.L.GPU_DestroyBuffer(self.buf)
            self.buf = None


class BorderedLevel:
    """A bordered source level on the device (pbrk_border_build from the plain level)."""

    def __init__(self, L, lvl):
        lvl = np.ascontiguousarray(lvl, dtype=np.float32)
        self.n_src = lvl.shape[1]
        pyr = DeviceBuffer(L, lvl.nbytes, lvl)
        self.dev = DeviceBuffer(L, 6 * (self.n_src + 2) ** 2 * 16, np.zeros((6, self.n_src + 2, self.n_src + 2, 4), np.float32))
        try:
            assert L.pbrk_border_build(pyr.ptr, self.dev.ptr, self.n_src, 1, None) == 0
        finally:
            pyr.free()                                                 # waits for the device first

    def free(self):
        self.dev.free()


_tables = {}


def prefilter_table(L, rough):
    """The reference's prefilter table for a roughness, on the device: (buffer, samples, alpha).  Kept for the process (a few
    hundred KB each)."""
    if rough not in _tables:
        tab = np.zeros((8192, 4), dtype=np.float32)
        alpha = C.c_float()
        n_tab = L.pbrk_host_prefilter_table(8192, rough, tab.ctypes.data_as(C.c_void_p), C.byref(alpha))
        assert 0 < n_tab <= 8192
        _tables[rough] = (DeviceBuffer(L, tab.nbytes, tab), n_tab, alpha.value)
    return _tables[rough]


def filter_windows(L, bord, rough, windows, out_size, n_tab=None):
    """pbrk_mc_filter once per window (face0, face1, y0, rows) of a BorderedLevel into one cleared cube of out_size^2 faces, with
    the first n_tab samples of the roughness's table (default: all).  Returns the cube's bytes.  Reads no counter, sets no switch."""
    dtab, n_full, alpha = prefilter_table(L, rough)
    zero = np.zeros((6, out_size, out_size, 4), np.float32)
    out = DeviceBuffer(L, zero.nbytes, zero)
    try:
        for f0, f1, y0, rows in windows:
            rc = L.pbrk_mc_filter(bord.dev.ptr, None, bord.n_src, dtab.ptr, n_tab or n_full, float(np.pi), alpha,
                                  out.ptr, out_size, f0, f1, y0, y0 + rows, None)
            assert rc == 0, rc
        return out.read()
    finally:
        out.free()


def env_texture(env):
    """A [6, W, W, 4] float32 environment as a mipmapped cube texture."""
    return pbrhip.make_texture(pbrhip.Format_RGBA32F, env.shape[1], env.shape[1],
                               pbrhip.TextureFlag_Cubemap | pbrhip.TextureFlag_HasMipmaps, env)


def digest(array):
    return hashlib.sha256(np.ascontiguousarray(array).view(np.uint8)).hexdigest()


@contextlib.contextmanager
def dispatch_prefilter_units(L, tex, S, units):
    """Fresh IBL maps with an S^2 specular cube, the counters zeroed, the work units recorded through PBR_RecordUnits, submitted and
    waited for.  Yields the maps: read levels and counters in the body, the maps are destroyed after it."""
    maps = pbrhip.PBR_IBLMaps()
    L.PBR_MakeIBLMaps(C.byref(maps), 8, 64, S)
    pipes = L.PBR_MakeIBLPipelines(); arena = L.GPU_MakeDescriptorArena(); g = L.GPU_MakeGraph()
    try:
        arr = (pbrhip.PBR_WorkUnit * len(units))(*units)
        reset_counters(L)
        L.PBR_RecordUnits(pipes, g, arena, tex, C.byref(maps), arr, len(units))
        L.GPU_GraphSubmit(g); L.GPU_GraphWait(g); L.GPU_ResetDescriptorArena(arena)
        yield maps
    finally:
        L.GPU_DestroyGraph(g); L.GPU_DestroyDescriptorArena(arena); L.PBR_DestroyIBLPipelines(pipes)
        L.PBR_DestroyIBLMaps(C.byref(maps))
