"""CPU tests of the ALS planner (plan_als, csrc/als_kernels.hip) through the host-only plan
query admmq_debug_cp_plan: the case table of oracle/als_bound.py plans the form each case is
there for, the table reaches every cell of {generic, spatial} x {BM 32, 64} x mode, split and
unsplit, and a ragged last K chunk; and the planner's refusals, none of which needs a GPU.
"""
import os

import numpy as np
import pytest

from oracle import als_bound as ab

ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libadmmq.so is not built: run __graft_entry__.build()")
    _lib.load()
    return _lib


def _plan(lib, c, mode, kind="mttkrp"):
    return lib.debug_cp_plan([(c["dims"], c["R"], ab.fake_address(c["band"]))], mode, kind)[0]


@pytest.mark.parametrize("case", ab.CASES, ids=ab.case_id)
def test_case_plans_its_form(lib, case):
    dims, R = case["dims"], case["R"]
    for mode, want in enumerate(case["plan"]):
        got = _plan(lib, case, mode)
        assert {k: got[k] for k in want} == want, (dims, R, mode, got)
        M = dims[mode] if got["job"] == ab.GENERIC or mode < 2 else dims[0]   # spatial mode 2 tiles over I
        assert got["tiles_m"] == -(-M // got["BM"]) and got["tiles_n"] == -(-R // 64)
        g = _plan(lib, case, mode, "gram")
        assert g == dict(job=ab.GRAM, BM=32 if R <= 32 else 64, tiles_m=-(-R // g["BM"]), tiles_n=-(-R // 64),
                         nsplit=1, kchunk=0), (dims, R, mode, g)


def test_table_reaches_every_cell(lib):
    """{generic, spatial} x {BM 32, 64} x the modes each admits (2-way and 3-way apart for the
    generic kernel), nsplit = 1 and > 1 for each kernel, a last chunk with K % 16 != 0."""
    want = {(job, BM, nd, m) for job, nds in ((ab.GENERIC, (2, 3)), (ab.SPATIAL, (3,))) for BM in (32, 64)
            for nd in nds for m in range(nd)}
    want |= {(job, split) for job in (ab.GENERIC, ab.SPATIAL) for split in ("unsplit", "split")}
    want |= {"ragged last chunk", "Khatri-Rao run across a chunk boundary", "2-way split on BM 32",
             "Gram BM 32 with Hadamard", "Gram BM 32 without", "Gram BM 64 with Hadamard", "Gram BM 64 without"}
    seen = set()
    for c in ab.CASES:
        dims, R = c["dims"], c["R"]
        for mode in range(len(dims)):
            p = _plan(lib, c, mode)
            seen.add((p["job"], p["BM"], len(dims), mode))
            seen.add((p["job"], "split" if p["nsplit"] > 1 else "unsplit"))
            g = _plan(lib, c, mode, "gram")
            seen.add(f"Gram BM {g['BM']} with{' Hadamard' if len(dims) == 3 else 'out'}")
            if p["job"] == ab.GENERIC and p["nsplit"] > 1:
                K = ab.n_terms(dims, mode)
                if (K - (p["nsplit"] - 1) * p["kchunk"]) % 16:
                    seen.add("ragged last chunk")
                K2 = 1 if len(dims) == 2 else (dims[1] if mode == 2 else dims[2])
                if p["kchunk"] % K2:
                    seen.add("Khatri-Rao run across a chunk boundary")
                if len(dims) == 2 and p["BM"] == 32:
                    seen.add("2-way split on BM 32")
    missing = want - seen
    assert not missing, f"the case table reaches no {sorted(map(str, missing))}"


def test_mixed_batch_holds_both_classes_and_kernels(lib):
    for mode in (0, 1, 2):
        sel = [(d, R, ab.fake_address(64)) for d, R in ab.MIXED if mode < len(d)]
        plans = lib.debug_cp_plan(sel, mode)
        assert plans == [lib.debug_cp_plan([L], mode)[0] for L in sel]   # a layer's form does not depend on the batch
        assert {p["job"] for p in plans} == {ab.GENERIC, ab.SPATIAL}, mode
        assert {p["BM"] for p in plans} == {32, 64}, mode
        if mode != 1:   # no reduction of mode 1 in this batch is long enough to split
            assert {p["nsplit"] > 1 for p in plans} == {False, True}, mode


def test_top_of_divmod_range_is_planned_in_short_chunks(lib):
    """oracle/als_bound.py (TOP): a reduction of nearly 2^24 terms is cut so that a term passes
    through at most 1 + kchunk + nsplit <= 10241 roundings."""
    for dims, R, plans in ab.TOP:
        for mode in range(3):
            p = lib.debug_cp_plan([(dims, R, ab.fake_address(64))], mode)[0]
            assert p["job"] == ab.GENERIC and p["BM"] == (32 if dims[mode] <= 32 else 64)
            assert 1 + min(p["kchunk"], ab.n_terms(dims, mode)) + p["nsplit"] <= 10241, (dims, mode, p)
            if mode in plans:
                assert (p["nsplit"], p["kchunk"]) == plans[mode], (dims, mode, p)
                assert ab.n_terms(dims, mode) > (1 << 22) and (p["nsplit"] - 1) * p["kchunk"] < ab.n_terms(dims, mode)


def test_divmod_model_on_the_tested_divisors():
    """divmod (csrc/als_kernels.hip) in numpy float32 over every k < 2^24: q = int(float(k) *
    (1.0f / d)) is within one of k / d, so one correction step each way is exact; and the
    divisors of the table that are there for the down-correction (3, 7, 33) do take it, so the
    GPU cases that name them run that branch."""
    k = np.arange(1 << 24, dtype=np.int64)
    kf = k.astype(np.float32)
    took_down = {}
    for d in (3, 5, 7, 9, 33, 64, 132, 150, 4099, 5592403):
        inv = np.float32(1.0) / np.float32(d)
        q = (kf * inv).astype(np.int64)          # float32 product, truncated like the C cast
        r = k - q * d
        assert r.min() >= -d and r.max() < 2 * d, d
        took_down[d] = int(np.count_nonzero(r < 0))
    print("k < 2^24 with the r < 0 correction:", took_down)
    assert took_down[3] > 1_000_000 and took_down[7] > 0 and took_down[33] > 0
    assert took_down[5] == 0 and took_down[9] == 0 and took_down[4099] == 0


def test_refusals(lib):
    a = ab.fake_address(64)
    rc = lambda dims, R, mode, kind="mttkrp": lib.debug_cp_plan([(dims, R, a)], mode, kind, raw=True)  # noqa: E731
    # Khatri-Rao index range >= 2^24 (divmod's exact range)
    assert rc((4096, 4096, 2), 3, 2) == ERR_ARG
    assert rc((1, 5592406, 3), 2, 0) == ERR_ARG
    assert b"2^24" in lib.load().admmq_last_error()
    assert rc((4096, 4095, 2), 3, 2) == 0
    assert rc((1, 5592403, 3), 2, 0) == 0
    assert rc((1, 5592406, 3), 2, 1) == 0            # mode 1 reduces over I Kd = 3 only
    assert rc((1, 5592406, 3), 2, 0, "error") == ERR_ARG   # the error's column index J Kd
    # bad mode, ndim, R
    assert rc((16, 16, 9), 5, 3) == ERR_ARG and rc((16, 16, 9), 5, -1) == ERR_ARG
    assert rc((16, 16), 5, 2) == ERR_ARG and rc((16, 16), 5, 2, "gram") == ERR_ARG
    assert rc((4, 4, 4, 4), 5, 0) == ERR_ARG
    assert rc((16, 16, 9), 0, 0) == ERR_ARG
    assert rc((16, 0, 9), 5, 0) == ERR_ARG
    assert lib.debug_cp_plan([((16, 16, 9), 5, 0)], 0, raw=True) == ERR_ARG   # NULL W
    assert rc((16, 16, 9), 5, 0) == 0
    assert lib.load().admmq_debug_cp_plan(None, 1, 0, 0, None) == ERR_ARG
    assert lib.load().admmq_debug_cp_plan(None, 0, 0, 0, None) == 0
    import ctypes
    out = (ctypes.c_int32 * 6)()
    arr = (lib.CpLayer * 1)()
    assert lib.load().admmq_debug_cp_plan(arr, 1, 0, 3, out) == ERR_ARG      # unknown kind
