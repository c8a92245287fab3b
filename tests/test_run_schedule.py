"""CPU test that pins the launch schedule of admmq_admm_run_ex: which launches a run call
makes is a pure function of the plan, the search form, the run switches and the call's
arguments (csrc/admm_plan.hip: search_form, schedule_run), and a refactor must not move one
field of it.

admmq_debug_admm_run_schedule plans against a fake workspace address (no device call; the
fused finalize's resident-block capacity is an argument) and returns the schedule's fields.
They are compared with tests/golden/run_schedules.json, written by
tests/golden/gen_run_schedules.py from the decisions as they stood inline in
admmq_admm_run_ex, and checked against what the conditions say by hand.
"""
import ctypes
import json
import os

import pytest

import gen_run_schedules as gen


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libadmmq.so is not built: run __graft_entry__.build()")
    return _lib.load()


@pytest.fixture(scope="module")
def computed(lib):
    """case name -> (arguments, schedule), computed once"""
    return {name: (args, sched) for name, args, sched in gen.cases(lib)}


def test_schedules_match_fixture(computed):
    with open(gen.FIXTURE) as f:
        want = json.load(f)
    assert tuple(want["slots"]) == gen.SLOTS and want["default"] == gen.DEFAULT
    want = want["schedules"]
    bad = []
    for name, (_, sched) in computed.items():
        got = [sched[s] for s in gen.SLOTS]
        if name not in want:
            bad.append(f"{name}: not in the fixture")
        elif got != want[name]:
            diff = {s: (a, b) for s, a, b in zip(gen.SLOTS, got, want[name]) if a != b}
            bad.append(f"{name}: (got, fixture) {diff}")
    assert not bad, f"{len(bad)} of {len(computed)} schedules differ:\n" + "\n".join(bad[:40])
    assert set(computed) == set(want), sorted(set(want) - set(computed))[:10]


def test_cases_cover_the_options(computed):
    """Every option is crossed with the named sets, the seeded batches only with the defaults."""
    opts = {name.split("/")[0] for name in computed}
    assert opts == set(gen.OPTIONS) and len(opts) == 16
    assert sum(name.startswith("default/random.") for name in computed) == 50
    assert not any("random." in name for name in computed if not name.startswith("default/"))


def test_schedule_invariants(computed):
    """What the conditions of schedule_run say, for every case."""
    for name, (a, s) in computed.items():
        fused_fin = s["search"] == gen.SEARCH_HIST3_FIN
        assert s["iters"] == max(a["max_iter"] - 1, 0), name
        assert s["zero_ready"] == fused_fin, name
        if not a["has_info"] or not a["fused_finalize"]:   # the paths that report through info never run
            assert not fused_fin and not s["zero_ready"] and not s["try_thin_loop"], name
        if a["max_iter"] == 1:
            assert s["iters"] == 0 and not s["try_thin_loop"], name
        if fused_fin:
            assert 0 < s["nh"] <= a["fin_capacity"] and s["nf"] == 0 and s["fin_wanted"], name
            assert s["search_list"] == gen.LIST_HIST, name
        if s["search"] == gen.SEARCH_HIST3:
            assert s["search_list"] == gen.LIST_HIST_MULTI and s["nh"] > 0, name
        if a["qscheme"] != gen.MSE:
            assert s["search"] == gen.SEARCH_NONE and s["nf"] == s["plan_nfin"], name
            assert not s["merged"] and not s["fuse_small"] and not s["try_thin_loop"], name
        else:
            assert (s["search"] == gen.SEARCH_ALL) == bool(s["exhaustive"]), name
            assert (s["search"] == gen.SEARCH_HIST) == (not s["exhaustive"] and not s["merged"]), name
        if s["exhaustive"]:
            assert not s["fuse_small"] and not s["merged"] and not s["try_thin_loop"], name
        if s["fuse_small"]:
            assert s["merged"] and s["nf"] < s["plan_nfin"], name
        elif not fused_fin:
            assert s["nf"] == s["plan_nfin"], name
        assert s["gemm"] or s["thin_solve"], name
        if not s["merged"]:
            assert s["ngroups"] == 0, name


def test_switches_take_the_other_form(computed):
    for name, (_, s) in computed.items():
        opt = name.split("/")[0]
        if opt in ("exhaustive=1", "bits=8", "num_attempts=1100"):
            assert s["exhaustive"] and s["search"] == gen.SEARCH_ALL, name
        if opt in ("legacy_stage1=1", "bits=6", "num_attempts=1"):
            assert not s["exhaustive"] and not s["merged"] and s["search"] == gen.SEARCH_HIST, name
        if opt in ("thin_loop=0", "has_info=0", "fused_finalize=0", "max_iter=1"):
            assert not s["try_thin_loop"], name
        if opt == "fin_capacity=0":
            assert s["search"] != gen.SEARCH_HIST3_FIN, name


def test_named_sets_pin_the_forms(computed, lib):
    _, s = computed["default/C3.mode2"]   # every factor thin: 4 bits, 200 candidates, info, 3 iterations
    assert s["try_thin_loop"] == 1 and s["thin_solve"] == 1 and s["gemm"] == gen.GEMM_NONE
    assert computed["max_iter=2/C3.mode2"][1]["try_thin_loop"] == 1
    a, s = computed["default/lone.512x1141"]
    assert a["fused_finalize"] == 1 and a["has_info"] == 1 and a["fin_capacity"] == 512
    assert s["search"] == gen.SEARCH_HIST3_FIN and s["zero_ready"] == 1 and s["nf"] == 0 and s["nh"] <= 512
    a, s = computed["fin_capacity=16/lone.512x1141"]
    assert a["fin_capacity"] == 16
    assert s["search"] == gen.SEARCH_HIST3 and s["zero_ready"] == 0 and s["nf"] == s["plan_nfin"] and s["nh"] > 0
    # the default K-split plans split tiles for C3 mode 0, none for the thin batch
    assert computed["default/C3.mode0"][1]["zero_kctr"] == 1 and computed["default/C3.mode2"][1]["zero_kctr"] == 0
    # the diagnostic fp32 kernels take the event-packet form of the GEMM marks
    assert lib.admmq_debug_set_f32_persistent(1, 1) == 0
    try:
        s = gen.schedule(lib, [(512, 1141)], **gen.DEFAULT)
    finally:
        assert lib.admmq_debug_set_f32_persistent(0, 1) == 0
    assert s["gemm"] == gen.GEMM_DIAG


def test_schedule_refuses_bad_arguments(lib):
    from admmq import _lib
    arr = _lib.problems_array([_lib.AdmmProblem(0, 0, 0, 0, 0, 0, 0, 64, 134)])
    out = (ctypes.c_int32 * 16)()

    def call(nprob=1, ncand=200, bits=4, scheme=0, solve=0, o=out):
        return lib.admmq_debug_admm_run_schedule(arr, nprob, ncand, bits, scheme, 4, solve, 1, 1, 512, o)

    assert call() == 0
    assert call(o=None) != 0 and call(solve=7) != 0 and call(scheme=9) != 0
    assert call(bits=0) != 0 and call(bits=17) != 0 and call(nprob=0) != 0 and call(ncand=0) != 0


class _Recorder:
    """Stands in for the library: records (setter, value) and answers `status`."""

    def __init__(self, status=0):
        self.calls, self.status = [], status

    def __getattr__(self, name):
        if name == "admmq_last_error":
            return lambda: b"refused"
        return lambda value: (self.calls.append((name, value)), self.status)[1]


# manager, its setter, (constructor arguments -> value on entry), value on exit, status checked (entry, exit)
SWITCH_MANAGERS = [
    ("exhaustive_search", "admmq_set_exhaustive_search", {(): 1, (True,): 1, (False,): 0}, 0, (False, False)),
    ("sel_widen", "admmq_debug_set_sel_widen", {(): 1}, 0, (True, True)),
    ("fin_nv3", "admmq_debug_set_fin_nv3", {(True,): 1, (False,): 0}, 1, (False, False)),
    ("fused_finalize", "admmq_debug_set_fused_finalize", {(True,): 1, (False,): 0}, 1, (False, False)),
    ("fin_wait_polls", "admmq_debug_set_fin_wait_polls", {(1,): 1, (4096,): 4096}, 0, (True, False)),
    ("fin_capacity", "admmq_debug_set_fin_capacity", {(16,): 16, (0,): 0}, 0, (True, False)),
    ("thin_loop", "admmq_debug_set_thin_loop", {(True,): 1, (False,): 0, ("wide",): 2}, 1, (True, False)),
    ("search_units_per_block", "admmq_debug_set_search_units_per_block", {(4,): 4, (0,): 0}, 0, (True, False)),
    ("stage1_form", "admmq_debug_set_legacy_stage1", {("legacy",): 1, ("merged",): 0}, 0, (False, False)),
]


@pytest.mark.parametrize("name,setter,enter,leave,checked", SWITCH_MANAGERS, ids=[m[0] for m in SWITCH_MANAGERS])
def test_switch_managers_set_and_restore(monkeypatch, name, setter, enter, leave, checked):
    """Each context manager of admmq._lib calls its setter with the encoded value on entry
    and the default on exit, and raises a refused setter's status only where it always did."""
    from admmq import _lib
    for args, value in enter.items():
        rec = _Recorder()
        monkeypatch.setattr(_lib, "load", lambda rec=rec: rec)
        with getattr(_lib, name)(*args) as cm:
            assert isinstance(cm, getattr(_lib, name)) and rec.calls == [(setter, value)]
        assert rec.calls == [(setter, value), (setter, leave)]
    args = next(iter(enter))
    rec = _Recorder(status=1)   # a setter that refuses
    monkeypatch.setattr(_lib, "load", lambda: rec)
    cm = getattr(_lib, name)(*args)
    if checked[0]:
        with pytest.raises(RuntimeError, match=name):
            cm.__enter__()
    else:
        cm.__enter__()
    if checked[1]:
        with pytest.raises(RuntimeError, match=name):
            cm.__exit__(None, None, None)
    else:
        assert cm.__exit__(None, None, None) is False
    with pytest.raises(ValueError):
        _lib.stage1_form("other")
