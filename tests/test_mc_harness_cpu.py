"""pbrhip.mc, the harness of the K4b tests and probes, against a fake library that records every call: which setters `switches`
calls and puts back, and in which order and with which reset flag `counters` reads the getters.  No library, no GPU."""
import pytest

from pbrhip import mc

# what the fake getters write into their slots, in slot order
SLOTS = {"pbrk_mc_region_stats": (3, 40), "pbrk_mc_region_skip_stats": (5, 6, 7), "pbrk_mc_region_flag_stats": (8, 9, 10),
         "pbrk_mc_region_window_stats": (11,), "pbrk_mc_launch_cut_stats": (12, 13, 14, 15, 16, 17),
         "pbrk_mc_region_phase_stats": (18, 19, 20, 21, 22)}


class FakeLib:
    """Records (name, args) of every call; a getter fills its buffer from SLOTS and returns 0, or -1 if it is in `failing`."""

    def __init__(self, failing=()):
        self.calls, self.failing = [], failing

    def __getattr__(self, name):
        def call(*args):
            if name in SLOTS:
                self.calls.append((name, args[1:]))                     # without the buffer
                if name in self.failing:
                    return -1
                args[0][:] = SLOTS[name]
                return 0
            self.calls.append((name, args))
        return call


def test_switches_set_the_named_and_restore_the_defaults():
    L = FakeLib()
    with mc.switches(L, absorb=0, tile32=1):
        assert L.calls == [("pbrk_mc_set_absorb", (0,)), ("pbrk_mc_set_tile32", (1,))]
        del L.calls[:]
    assert L.calls == [("pbrk_mc_set_absorb", (1,)), ("pbrk_mc_set_tile32", (-1,))]      # and no switch that was not named


def test_switches_restore_when_the_body_raises():
    L = FakeLib()
    with pytest.raises(ZeroDivisionError):
        with mc.switches(L, absorb=0, tile32=1):
            del L.calls[:]
            1 / 0
    assert L.calls == [("pbrk_mc_set_absorb", (1,)), ("pbrk_mc_set_tile32", (-1,))]


def test_every_switch_and_its_default():
    L = FakeLib()
    with mc.switches(L, absorb=0, runs=0, prologue=0, launch_cut=0, tile32=0, kernels=(0, 1)):
        assert ("pbrk_mc_set_kernels", (0, 1)) in L.calls and len(L.calls) == 6
        del L.calls[:]
    assert sorted(L.calls) == sorted([("pbrk_mc_set_absorb", (1,)), ("pbrk_mc_set_runs", (1,)), ("pbrk_mc_set_prologue", (1,)),
                                      ("pbrk_mc_set_launch_cut", (1,)), ("pbrk_mc_set_tile32", (-1,)), ("pbrk_mc_set_kernels", (-1, -1))])


def test_unknown_switch_is_a_type_error():
    L = FakeLib()
    with pytest.raises(TypeError):
        with mc.switches(L, absorb=0, tile64=1):
            pass
    assert L.calls == []


def test_region_is_read_last_and_alone_takes_the_reset():
    L = FakeLib()
    c = mc.counters(L, "region", "skip", reset=True)
    assert L.calls == [("pbrk_mc_region_skip_stats", ()), ("pbrk_mc_region_stats", (1,))]
    assert c == {"abs_words": 5, "abs_samples": 6, "count_only": 7, "healed": 3, "slices": 40}
    del L.calls[:]
    mc.counters(L, "region")
    assert L.calls == [("pbrk_mc_region_stats", (0,))]


def test_keys_of_every_group():
    L = FakeLib()
    c = mc.counters(L, "phase", "cut", "region", "window", "flag", "skip")
    assert [n for n, _ in L.calls][-1] == "pbrk_mc_region_stats" and len(L.calls) == 6
    assert c == {"healed": 3, "slices": 40, "abs_words": 5, "abs_samples": 6, "count_only": 7, "flags": 8, "flag_samples": 9, "visits": 10,
                 "proved": 11, "cut4": [12, 13, 14, 15], "nw": 16, "words_cut": 17, "phase": (18, 19, 20, 21, 22)}


def test_failing_getter_raises_unless_missing_ok():
    L = FakeLib(failing=("pbrk_mc_launch_cut_stats",))
    with pytest.raises(AssertionError, match="pbrk_mc_launch_cut_stats"):
        mc.counters(L, "cut", "region")
    c = mc.counters(L, "cut", "region", missing_ok=True)
    assert c == {"healed": 3, "slices": 40}


def test_reset_counters_ignores_the_return_code():
    L = FakeLib(failing=("pbrk_mc_region_stats",))
    mc.reset_counters(L)
    assert L.calls == [("pbrk_mc_region_stats", (1,))]
