"""The cases of tests/test_run_schedule.py and the generator of its fixture.

    python tests/golden/gen_run_schedules.py       # rewrites tests/golden/run_schedules.json

Every case is one call of admmq_debug_admm_run_schedule: the launch schedule that
admmq_admm_run_ex follows for a batch of (I, R) factors (the 16 slots named in SLOTS; the
layout is documented beside the entry point in csrc/api.hip). The fixture was written by the
decisions as they stood inline in admmq_admm_run_ex, before they moved into search_form and
schedule_run (csrc/admm_plan.hip); it is regenerated only by a change that means to alter a
schedule, never to make a refactor pass.
"""
import ctypes
import json
import os
import sys

import gen_plan_digests as plans

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "run_schedules.json")
SLOTS = ("iters", "try_thin_loop", "zero_kctr", "zero_ready", "gemm", "thin_solve", "search", "search_list", "nh",
         "fuse_small", "nf", "exhaustive", "merged", "ngroups", "fin_wanted", "plan_nfin")
# the values of the "gemm", "search" and "search_list" slots
GEMM_NONE, GEMM_TILES, GEMM_DIAG = 0, 1, 2
SEARCH_NONE, SEARCH_HIST3, SEARCH_HIST3_FIN, SEARCH_HIST, SEARCH_ALL = 0, 1, 2, 3, 4
LIST_HIST, LIST_HIST_MULTI = 0, 1
MSE, MINMAX = 0, 1

DEFAULT = dict(qscheme=MSE, bits=4, max_iter=4, fused_finalize=1, has_info=1, fin_capacity=512, num_attempts=200)
# option name -> (arguments that differ from DEFAULT, process switch (setter, value, restore) or None)
OPTIONS = {"default": ({}, None)}
OPTIONS["qscheme=minmax"] = (dict(qscheme=MINMAX), None)
for _b in (1, 6, 8):
    OPTIONS[f"bits={_b}"] = (dict(bits=_b), None)
for _m in (1, 2):
    OPTIONS[f"max_iter={_m}"] = (dict(max_iter=_m), None)
OPTIONS["fused_finalize=0"] = (dict(fused_finalize=0), None)
OPTIONS["has_info=0"] = (dict(has_info=0), None)
for _c in (0, 16):
    OPTIONS[f"fin_capacity={_c}"] = (dict(fin_capacity=_c), None)
OPTIONS["exhaustive=1"] = ({}, ("admmq_set_exhaustive_search", 1, 0))
OPTIONS["legacy_stage1=1"] = ({}, ("admmq_debug_set_legacy_stage1", 1, 0))
OPTIONS["thin_loop=0"] = ({}, ("admmq_debug_set_thin_loop", 0, 1))
for _n in (1, 1100):
    OPTIONS[f"num_attempts={_n}"] = (dict(num_attempts=_n), None)


def schedule(lib, batch, *, qscheme, bits, max_iter, fused_finalize, has_info, fin_capacity, num_attempts,
             solve_mode=0):
    """The schedule of one call as {slot name: value}."""
    from admmq import _lib
    arr = _lib.problems_array([_lib.AdmmProblem(0, 0, 0, 0, 0, 0, 0, i, r) for i, r in batch])
    out = (ctypes.c_int32 * 16)()
    rc = lib.admmq_debug_admm_run_schedule(arr, len(batch), num_attempts, bits, qscheme, max_iter, solve_mode,
                                           fused_finalize, has_info, fin_capacity, out)
    assert rc == 0, lib.admmq_last_error()
    return dict(zip(SLOTS, (int(v) for v in out)))


def cases(lib):
    """Yields (case name, the call's arguments, its schedule). The default arguments: the
    named sets and the first 50 seeded batches; every other option, one at a time: the named
    sets only."""
    named = plans.shape_sets()
    for oname, (diff, switch) in OPTIONS.items():
        args = {**DEFAULT, **diff}
        sets = {**named, **plans.random_sets(50)} if oname == "default" else named
        if switch:
            assert getattr(lib, switch[0])(switch[1]) == 0, oname
        try:
            for name, batch in sets.items():
                yield f"{oname}/{name}", args, schedule(lib, batch, **args)
        finally:
            if switch:
                assert getattr(lib, switch[0])(switch[2]) == 0, oname


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    for p in (root, os.path.join(root, "admm-quantization_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from admmq import _lib
    lib = _lib.load()
    out = {name: [sched[s] for s in SLOTS] for name, _, sched in cases(lib)}
    with open(FIXTURE, "w") as f:   # one case per line
        f.write(f'{{"slots": {json.dumps(SLOTS)}, "default": {json.dumps(DEFAULT)}, "schedules": {{\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(out.items())))
        f.write("\n}}\n")
    print(f"{len(out)} cases -> {FIXTURE}")


if __name__ == "__main__":
    main()
