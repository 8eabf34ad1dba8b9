"""mc_plan (csrc/mc_plan.cpp), the one function that decides which kernels serve a pbrk_mc_filter dispatch, against the dispatch the
library made BEFORE the plan existed: tests/golden/mc_plan_kernels.json holds, per case, the ordered kernel names of a kernel trace of
that library (one process with the device counters off, one with PBR_MC_STATS=1; a fresh bordered level per case, the table registered
with the bin cache).  No GPU: pbrk_mc_plan is asked with the case's level, window, switches and counters, and must name the same
k_mc_region / k_mc_resident instantiation (or, declining, the same k_mc_filter_lds / k_mc_filter one), the same k_mc_prep and k_mc_cut ahead of it
and the same k_mc_refine_bins behind it.  The bin cache's state is an input: "cache": "clear" is a first launch, "keep" finds the entry
of the case before it."""
import contextlib
import json
import os

import pytest

import pbrhip
from pbrhip import mc

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mc_plan_kernels.json")) as _f:
    CASES = json.load(_f)


@contextlib.contextmanager
def case_switches(L, named):
    named = {k: tuple(v) if isinstance(v, list) else v for k, v in named.items()}
    resident = named.pop("resident", None)
    if resident is not None:
        L.pbrk_mc_set_resident(resident)
    try:
        with mc.switches(L, **named):
            yield
    finally:
        L.pbrk_mc_set_resident(-1)


def test_fixture_covers_the_issue_list():
    assert len(CASES) == 258 and {c["counters"] for c in CASES} == {0, 1}
    seen = {k.split("<")[0] for c in CASES for k in c["kernels"]}
    assert seen == {"k_mc_region", "k_mc_resident", "k_mc_refine_bins", "k_mc_prep", "k_mc_cut", "k_mc_filter", "k_mc_filter_lds"}
    assert all(len([k for k in c["kernels"] if k.startswith(("k_mc_region", "k_mc_resident", "k_mc_filter"))]) == 1 for c in CASES)


@pytest.mark.parametrize("counters", [0, 1])
def test_plan_names_the_recorded_kernels(counters):
    L = pbrhip.lib()
    wrong = []
    for c in CASES:
        if c["counters"] != counters:
            continue
        f0, f1, y0, rows = c["window"]
        with case_switches(L, c["switches"]):
            p = mc.plan(L, c["n_src"], c["n_tab"], c["size"], window=(f0, f1, y0, rows), counters=bool(counters), have_prep=True)
        got = c["kernels"]
        records = p["bin_cache"] and p["bin_eligible"] and p["whole"] and c["cache"] == "clear"
        if p["family"] == "declined":
            want = [p["kernel"]]                                           # the level-in-LDS or the direct kernel
        else:
            want = ["k_mc_prep"] * p["prep"] + ["k_mc_cut"] * p["cut"] + [p["kernel"]] + [p["refine_kernel"]] * bool(records and p["refine"])
        if want != got:
            wrong.append((c["name"], want, got))
    assert not wrong, f"{len(wrong)} cases, the first: {wrong[:3]}"


def test_no_prep_slot_is_a_plan_input():
    """The one runtime fallback (stream capture, no device memory): no k_mc_prep slot means the earlier prologue, no cut, and only the
    34^2 shape stays bin-eligible."""
    L = pbrhip.lib()
    for n_src, eligible in ((32, 1), (64, 0), (128, 0)):
        with_slot, without = (mc.plan(L, n_src, 160, 256, have_prep=h) for h in (True, False))
        assert without["prep"] == 0 and without["cut"] == 0 and without["bin_eligible"] == eligible
        assert without["lean"] == (1 if n_src == 32 else 0) and with_slot["lean"] == 1
        assert {k: v for k, v in without.items() if k in ("RS", "G", "RC", "NR", "NW", "tile", "lds", "expect", "absorb")} == \
               {k: v for k, v in with_slot.items() if k in ("RS", "G", "RC", "NR", "NW", "tile", "lds", "expect", "absorb")}
