"""The buffer-size policy of an alignment pass (kaptive_amd/csrc/kp_caps.h), built with g++ and checked on the CPU.

Every expected value is worked out by hand from the policy's arithmetic for a batch of 4 assemblies and 25000 packed
words, with 64 anchor sub-slices per assembly; the values are asserted exactly (cand_frac, a double, to 1e-12)."""

from __future__ import annotations

import ctypes as C

import pytest

from tests.harness_util import build_harness

N_ASM, TOTAL_WORDS = 4, 25000
FITTED, GREW, OVERFLOW = 0, 1, 2
u32, u64, i64 = C.c_uint32, C.c_uint64, C.c_int64


class _Struct(C.Structure):
    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Options(_Struct):
    _fields_ = [("anchor_cap", u32), ("tasks_per_asm", u32), ("hit_cap", u32), ("trace_kb_per_asm", u32), ("cand_cap", u64),
                ("group_cap", u32), ("join_cap", u32), ("occ_slots", u32), ("trace_set", C.c_bool), ("kept_cap", u32),
                ("piece_cap", u32), ("prot_cap", u32)]  # fmt: skip


class Learnt(_Struct):
    _fields_ = [("anchor_cap", u32), ("hit_cap", u32), ("tasks_per_asm", u32), ("cand_frac", C.c_double), ("words_hw", i64),
                ("trace_units_per_asm", u64), ("group_cap", u32), ("join_cap", u32), ("occ_slots", u32)]  # fmt: skip


class PassCaps(_Struct):
    _fields_ = [("anchor_cap", u32), ("task_cap", u32), ("hit_cap", u32), ("cand_cap", u64), ("trace_cap", u64),
                ("group_cap", u32), ("join_cap", u32), ("occ_slots", u32)]  # fmt: skip


class Seen(_Struct):
    _fields_ = [("n_cand", u64), ("trace_need", u64), ("occ_need", u64), ("max_slice", u32), ("max_task", u32),
                ("n_group", u32), ("max_join", u32), ("n_asm", u64), ("total_words", i64)]  # fmt: skip


@pytest.fixture(scope="module")
def lib():
    lib = build_harness("caps_harness", "kp_caps.h")
    layout = (C.c_int32 * 6)()
    lib.kpc_layout(layout)
    assert list(layout) == [C.sizeof(Options), C.sizeof(Learnt), C.sizeof(PassCaps), C.sizeof(Seen), 64, 65536]
    return lib


def default_options(lib) -> Options:
    o = Options()
    lib.kpc_default_options(C.byref(o))
    return o


def seen(**kw) -> Seen:
    return Seen(n_asm=N_ASM, total_words=TOTAL_WORDS, **kw)


def after_pass(lib, learnt: Learnt, caps: PassCaps, s: Seen):
    msg = C.create_string_buffer(512)
    verdict = lib.kpc_after_pass(C.byref(learnt), C.byref(caps), C.byref(s), msg, 512)
    return verdict, msg.value.decode()


def test_sizing_from_default_options(lib):
    learnt, caps = Learnt(), PassCaps()
    lib.kpc_size(C.byref(default_options(lib)), C.byref(learnt), N_ASM, i64(TOTAL_WORDS), C.byref(caps))
    assert caps.as_dict() == dict(anchor_cap=131072, task_cap=4 * 4096, hit_cap=4096, cand_cap=65536, trace_cap=4 * 131072,
                                  group_cap=1024, join_cap=1024, occ_slots=2)  # fmt: skip
    # the learnt 25390 words * 4 * 0.004 = 406 candidates lie under the floor of 65536
    assert learnt.as_dict() == dict(anchor_cap=131072, hit_cap=4096, tasks_per_asm=4096, cand_frac=0.004, words_hw=25390,
                                    trace_units_per_asm=131072, group_cap=1024, join_cap=1024, occ_slots=2)  # fmt: skip


def test_sizing_keeps_sixteen_anchors_a_sub_slice(lib):
    o, learnt, caps = default_options(lib), Learnt(), PassCaps()
    o.anchor_cap = 1
    lib.kpc_size(C.byref(o), C.byref(learnt), N_ASM, i64(TOTAL_WORDS), C.byref(caps))
    assert caps.anchor_cap == 1024 and learnt.anchor_cap == 1024


SMALL = dict(cand_cap=1, anchor_cap=1024, trace_cap=64, group_cap=1, join_cap=1, occ_slots=1, task_cap=4)
ROOMY = dict(cand_cap=10**6, anchor_cap=64 * 1000, trace_cap=10**6, group_cap=1000, join_cap=1000, occ_slots=100, task_cap=10**5)
OBSERVED = dict(n_cand=1000, max_slice=100, trace_need=1000, n_group=100, max_join=100, occ_need=5, max_task=5000)
# list -> (pass caps, learnt values) after the overflow branch
GROWN = {
    "cand_cap": (dict(cand_cap=1125), dict(cand_frac=1125 / 100000 * 1.0001)),
    "anchor_cap": (dict(anchor_cap=10240), dict(anchor_cap=10240)),
    "trace_cap": (dict(trace_cap=1250), dict(trace_units_per_asm=313)),
    "group_cap": (dict(group_cap=189), dict(group_cap=189)),
    "join_cap": (dict(join_cap=189), dict(join_cap=189)),
    "occ_slots": (dict(occ_slots=7), dict(occ_slots=7)),
    "task_cap": (dict(task_cap=6144), dict(tasks_per_asm=1536)),
}


def assert_state(learnt: Learnt, caps: PassCaps, want_learnt: dict, want_caps: dict):
    """`want_learnt` names the learnt values that differ from a fresh context's."""
    got, want = learnt.as_dict(), {**Learnt().as_dict(), **want_learnt}
    assert got.pop("cand_frac") == pytest.approx(want.pop("cand_frac"), rel=1e-12, abs=0.0)
    assert got == want
    assert caps.as_dict() == want_caps


def test_every_list_overflowing_grows(lib):
    learnt, caps = Learnt(), PassCaps(hit_cap=4096, **SMALL)
    verdict, _ = after_pass(lib, learnt, caps, seen(**OBSERVED))
    assert verdict == GREW
    want_caps, want_learnt = dict(hit_cap=4096), {}
    for c, l in GROWN.values():
        want_caps.update(c)
        want_learnt.update(l)
    assert_state(learnt, caps, want_learnt, want_caps)


@pytest.mark.parametrize("which", list(GROWN))
def test_one_list_overflowing_changes_only_its_own(lib, which):
    start = {**ROOMY, which: SMALL[which]}
    learnt, caps = Learnt(), PassCaps(hit_cap=4096, **start)
    verdict, _ = after_pass(lib, learnt, caps, seen(**OBSERVED))
    assert verdict == GREW
    assert_state(learnt, caps, dict(GROWN[which][1]), {**start, "hit_cap": 4096, **GROWN[which][0]})


def test_limits(lib):
    learnt, caps = Learnt(), PassCaps(**ROOMY)
    verdict, msg = after_pass(lib, learnt, caps, seen(trace_need=2**32 + 1))
    assert verdict == OVERFLOW and msg == "DP trace would exceed 64 GB; use smaller batches"
    learnt, caps = Learnt(), PassCaps(**{**ROOMY, "occ_slots": 65536})
    verdict, msg = after_pass(lib, learnt, caps, seen(occ_need=65537))
    assert verdict == OVERFLOW
    assert msg == ("occurrence-cut tables overflowed: 65537 assemblies of the batch need their own mid_occ, at most 65536 tables; "
                   "use smaller batches")  # fmt: skip
    learnt, caps = Learnt(), PassCaps(**{**ROOMY, "occ_slots": 2})
    verdict, _ = after_pass(lib, learnt, caps, seen(occ_need=65537))
    assert verdict == GREW and learnt.occ_slots == 65536 and caps.occ_slots == 65536


# pass cap, what the pass observed -> the learnt quantity afterwards (None: unchanged)
HEADROOM = [
    (dict(anchor_cap=6400), dict(max_slice=90), dict(anchor_cap=9216)),
    (dict(anchor_cap=6400), dict(max_slice=80), None),
    (dict(group_cap=100), dict(n_group=90), dict(group_cap=180)),
    (dict(group_cap=100), dict(n_group=80), None),
    (dict(join_cap=100), dict(max_join=90), dict(join_cap=180)),
    (dict(join_cap=100), dict(max_join=80), None),
    (dict(trace_cap=1000), dict(trace_need=950), dict(trace_units_per_asm=297)),
    (dict(trace_cap=1000), dict(trace_need=900), None),
    (dict(task_cap=1000), dict(max_task=950), dict(tasks_per_asm=297)),
    (dict(task_cap=1000), dict(max_task=900), None),
    (dict(cand_cap=1000), dict(n_cand=950), dict(cand_frac=(950 + 237) / 100000)),
    (dict(cand_cap=1000), dict(n_cand=900), None),
]


@pytest.mark.parametrize("cap,observed,want", HEADROOM)
def test_fitted_pass_adds_headroom_where_it_came_close(lib, cap, observed, want):
    start = {**ROOMY, **cap}
    learnt, caps = Learnt(), PassCaps(**start)
    verdict, _ = after_pass(lib, learnt, caps, seen(**observed))
    assert verdict == FITTED
    assert_state(learnt, caps, dict(want or {}), {**start, "hit_cap": 0})  # the pass's own caps stay as they are


def test_learnt_values_never_shrink(lib):
    learnt, caps = Learnt(group_cap=500), PassCaps(**{**ROOMY, "group_cap": 100})
    verdict, _ = after_pass(lib, learnt, caps, seen(n_group=90))
    assert verdict == FITTED and learnt.group_cap == 500


def test_hit_cap_growth(lib):
    learnt, caps = Learnt(hit_cap=256), PassCaps(hit_cap=256)
    lib.kpc_grow_hits(C.byref(learnt), C.byref(caps), u32(1000), 1)
    assert (caps.hit_cap, learnt.hit_cap) == (1280, 1280)  # (1000 + 250 + 255) & ~255
    learnt, caps = Learnt(hit_cap=2048), PassCaps(hit_cap=256)
    lib.kpc_grow_hits(C.byref(learnt), C.byref(caps), u32(1000), 0)  # hits a caller set: rounded up only
    assert (caps.hit_cap, learnt.hit_cap) == (1024, 2048)


def test_reduction_caps(lib):
    caps3, msg = (C.c_int32 * 3)(256, 32, 32768), C.create_string_buffer(256)
    assert lib.kpc_grow_run(caps3, 1, msg, 256) == 1 and list(caps3) == [1024, 32, 32768]
    assert lib.kpc_grow_run(caps3, 1, msg, 256) == 1 and list(caps3) == [2048, 32, 32768]
    assert lib.kpc_grow_run(caps3, 1 | 2 | 8, msg, 256) == 0 and list(caps3) == [2048, 32, 32768]
    assert msg.value.decode() == "more than 2048 non-overlapping hits in one assembly"
    assert lib.kpc_grow_run(caps3, 2, msg, 256) == 1 and list(caps3) == [2048, 128, 32768]
    assert lib.kpc_grow_run(caps3, 8, msg, 256) == 1 and list(caps3) == [2048, 128, 131072]


LEARNT_OF = dict(anchor_cap="anchor_cap", tasks_per_asm="tasks_per_asm", hit_cap="hit_cap", trace_kb_per_asm="trace_units_per_asm",
                 cand_cap="cand_frac", group_cap="group_cap", join_cap="join_cap", occ_slots="occ_slots")  # fmt: skip


@pytest.mark.parametrize("name", list(LEARNT_OF) + ["kept_cap", "piece_cap", "prot_cap"])
def test_set_option_resets_only_its_own_learnt_value(lib, name):
    full = dict(anchor_cap=6400, hit_cap=512, tasks_per_asm=77, cand_frac=0.25, words_hw=9, trace_units_per_asm=88,
                group_cap=5, join_cap=6, occ_slots=7)  # fmt: skip
    o, learnt, runs = default_options(lib), Learnt(**full), (C.c_int32 * 6)(1, 2, 3, 4, 5, 6)
    before = o.as_dict()
    assert lib.kpc_set_option(C.byref(o), C.byref(learnt), runs, 2, name.encode(), i64(12)) == 1
    want_runs = [1, 2, 3, 4, 5, 6]
    if name in LEARNT_OF:
        full[LEARNT_OF[name]] = 0
    else:
        k = ["kept_cap", "piece_cap", "prot_cap"].index(name)
        want_runs[k] = want_runs[3 + k] = 0
    assert learnt.as_dict() == full and list(runs) == want_runs
    assert o.as_dict() == {**before, name: 12, "trace_set": name == "trace_kb_per_asm"}


def test_set_option_bounds_and_unknown_names(lib):
    o, learnt, runs = default_options(lib), Learnt(occ_slots=3), (C.c_int32 * 3)(1, 2, 3)
    assert lib.kpc_set_option(C.byref(o), C.byref(learnt), runs, 1, b"occ_slots", i64(10**6)) == 1 and o.occ_slots == 65536
    assert lib.kpc_set_option(C.byref(o), C.byref(learnt), runs, 1, b"anchor_cap", i64(0)) == 1 and o.anchor_cap == 1
    before = (o.as_dict(), learnt.as_dict(), list(runs))
    assert lib.kpc_set_option(C.byref(o), C.byref(learnt), runs, 1, b"scan_mode", i64(1)) == 0
    assert (o.as_dict(), learnt.as_dict(), list(runs)) == before
