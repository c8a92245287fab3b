"""CPU test that pins the ADMM launch planner: the plan is a pure function of the problems'
shapes, the switches, the solve mode and the CU count, and a refactor of the planner must
not move one field of it.

admmq_debug_admm_plan_digest runs the planner as admmq_admm_prepare_ex would against a fake
workspace address (never dereferenced, no device call) and returns one digest per section
of the plan; they are compared with tests/golden/plan_digests.json, written by
tests/golden/gen_plan_digests.py from the planner as it stood inside api.hip. A mismatch
names the case and the sections that differ.

Without a device the planner's CU count answers 256. That is the MI355X's own count, so the
same fixture holds on the GPU machine.
"""
import json
import os

import pytest

import gen_plan_digests as gen


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libadmmq.so is not built: run __graft_entry__.build()")
    return _lib.load()


def test_random_batches_cover_every_kind():
    """The seeded batches hold thin, 32-row, 64 x 64 and tall factors and R above 1152."""
    flat = [ir for batch in gen.random_sets().values() for ir in batch]
    assert any(i <= 16 for i, _ in flat) and any(16 < i <= 32 for i, _ in flat)
    assert any(32 < i <= 64 for i, _ in flat) and any(i > 700 for i, _ in flat)
    assert any(r > 1152 for _, r in flat) and any(r % 32 for _, r in flat)


def test_plan_digests_match_fixture(lib):
    with open(gen.FIXTURE) as f:
        want = json.load(f)
    assert want["num_attempts"] == gen.NCAND and tuple(want["sections"]) == gen.SECTIONS
    want = want["digests"]
    seen, bad = set(), []
    for name, first, second in gen.cases(lib):
        seen.add(name)
        if first != second:   # the tile memo's miss against its hit
            bad.append(f"{name}: two calls in a row differ")
        elif name not in want:
            bad.append(f"{name}: not in the fixture")
        elif first != want[name]:
            diff = [s for s, a, b in zip(gen.SECTIONS, first, want[name]) if a != b]
            bad.append(f"{name}: sections {diff} differ")
    assert not bad, f"{len(bad)} of {len(seen)} plans differ:\n" + "\n".join(bad[:40])
    assert seen == set(want), sorted(set(want) - seen)[:10]


def test_digest_refuses_bad_arguments(lib):
    import ctypes
    from admmq import _lib
    arr = _lib.problems_array([_lib.AdmmProblem(0, 0, 0, 0, 0, 0, 0, 64, 134)])
    out = (ctypes.c_uint64 * 8)()
    assert lib.admmq_debug_admm_plan_digest(arr, 1, 200, 0, None, out) != 0
    assert lib.admmq_debug_admm_plan_digest(arr, 1, 200, 7, ctypes.c_void_p(gen.BASE), out) != 0
    assert lib.admmq_debug_admm_plan_digest(arr, 0, 200, 0, ctypes.c_void_p(gen.BASE), out) != 0
