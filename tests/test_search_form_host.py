"""CPU test of the search-form table: which device form the MSE-minmax search takes for
every (bits, num_attempts) (csrc/admm_plan.hip: two_stage_ok, merged_tables, search_form;
csrc/mse_search.hip: merged_ok and the launch_mse_* dispatchers).

The rule is restated here in Python and compared with what admmq_debug_admm_run_schedule
reports (no device call), for bits 1..8 x the candidate counts of the F13 matrix on a tall,
a thin and a mixed batch. The merged-threshold stage 1 (k_mse_hist3, k_mse_small_admm) is
instantiated for QMAX = 2^(bits-1) = 1, 2, 4, 8, 16 only, so it may be reported for 1..5
bits and nothing else: at 6 bits the host would build its tables for 32 levels and the
kernel read them as 16, scoring a 5-bit quantizer in stage 1.
"""
import collections
import os

import pytest

import gen_run_schedules as gen
import golden_cases as gc

ATTEMPTS = sorted(set(gc.F13_ATTEMPTS) | {na for _, na in gc.F13_EXTRA})   # 1 2 50 64 128 196 200 201 1100
BITS = range(1, 9)
BATCHES = {"tall": [(40, 134)], "thin": [(9, 134)], "mixed": [(40, 134), (64, 278), (9, 134)]}

# admmq_internal.h / mse_search.hip
MAX_STAGE1, MAX_STAGE1_BITS, MAX_MERGED, CELLS, TSORT_PAD, SSE_QUADS, MAX_TIE, TL_MAX_CAND = 1024, 6, 4096, 4096, 4, 512, 4, 256
MERGED_QMAX = {1: 1, 2: 2, 3: 4, 4: 8, 5: 16}   # bits -> the QMAX instantiations of k_mse_hist3 / k_mse_small_admm


def hist_lds_bytes(n, bits):
    qmax = 1 << (bits - 1)
    nb = n + 1 + 64
    thr = max(qmax * n * 4, (n + 1) * 8)
    return max(nb * 8 + ((nb + 3) & ~3) * 4 + thr, SSE_QUADS * 16)


def hist3_lds_bytes(n, bits):
    m = n << (bits - 1)
    nb = m + 1 + 64
    b = nb * (8 + 8 + 4 + 4) + m * 8 + TSORT_PAD * 4 + (((m + 1) & ~1) + CELLS + 2) * 2 + n * 4
    return max((b + 15) & ~15, SSE_QUADS * 16)


def two_stage_ok(n, bits):
    return n <= MAX_STAGE1 and bits <= MAX_STAGE1_BITS and hist_lds_bytes(n, bits) <= 64 * 1024


def tie_groups(n, qmax):
    """Sizes of the groups of equal threshold keys (2k-1) ((n-1) + 5c), k = 1..qmax, c < n."""
    keys = collections.Counter((2 * k - 1) * ((n - 1) + 5 * c) for k in range(1, qmax + 1) for c in range(n))
    return [v for v in keys.values() if v > 1]


def merged_rule(n, bits):
    """(merged, ngroups) for the default switches and the MSE scheme."""
    ok = (two_stage_ok(n, bits) and bits in MERGED_QMAX and n >= 2 and (n << (bits - 1)) <= MAX_MERGED and
          hist3_lds_bytes(n, bits) <= 150 * 1024)
    if not ok:
        return False, 0
    g = tie_groups(n, MERGED_QMAX[bits])
    return (True, len(g)) if max(g, default=0) <= MAX_TIE else (False, 0)


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libadmmq.so is not built: run __graft_entry__.build()")
    return _lib.load()


@pytest.fixture(scope="module")
def table(lib):
    """(batch, bits, na) -> schedule, computed once"""
    return {(name, bits, na): gen.schedule(lib, batch, **{**gen.DEFAULT, "bits": bits, "num_attempts": na})
            for name, batch in BATCHES.items() for bits in BITS for na in ATTEMPTS}


def test_restated_rule_names_the_cells():
    """The cells the matrix is built around, by the restated rule alone."""
    assert not merged_rule(196, 4)[0] and not merged_rule(201, 4)[0] and not merged_rule(196, 5)[0]   # a tie group of 5
    assert merged_rule(200, 4) == (True, 5) and merged_rule(200, 5) == (True, 66)
    assert not merged_rule(1, 4)[0] and two_stage_ok(1, 4)
    assert not two_stage_ok(1100, 4) and not two_stage_ok(200, 7)
    # 6 bits: the size and tie-group limits alone would admit 105 candidate counts up to 128
    # (every n = 1 mod 5 from 21 on has a tie group above 4); only the missing instantiation refuses them
    fits = [n for n in range(2, 129) if max(tie_groups(n, 32), default=0) <= MAX_TIE]
    assert len(fits) == 105 and {50, 64, 100, 128} <= set(fits)
    assert not [n for n in range(21, 129, 5) if n in fits]
    assert not any(merged_rule(n, 6)[0] for n in range(1, 1025))


def test_reported_form_equals_the_rule(table):
    bad = []
    for (name, bits, na), s in table.items():
        merged, ngroups = merged_rule(na, bits)
        want = (int(not two_stage_ok(na, bits)), int(merged), ngroups)
        got = (s["exhaustive"], s["merged"], s["ngroups"])
        if got != want:
            bad.append(f"{name} bits={bits} na={na}: (exhaustive, merged, ngroups) {got}, the rule {want}")
    assert not bad, f"{len(bad)} of {len(table)} cells differ:\n" + "\n".join(bad[:40])


def test_merged_only_where_instantiated(table):
    bad = [key for key, s in table.items() if s["merged"] and key[1] not in MERGED_QMAX]
    assert not bad, f"merged stage 1 reported for a width without a QMAX = 2^(bits-1) kernel: {bad}"


def test_schedule_follows_the_form(table):
    """The launches that follow from the form: the exhaustive sweep, the per-level stage 1 or
    the merged one (with the one-block kernel for the thin factors), and the persistent loop
    for an all-thin batch at 2..5 bits and 2..256 candidates only."""
    for (name, bits, na), s in table.items():
        key = (name, bits, na)
        if s["exhaustive"]:
            assert s["search"] == gen.SEARCH_ALL and not s["fuse_small"], key
        elif not s["merged"]:
            assert s["search"] == gen.SEARCH_HIST and s["nh"] > 0 and not s["fuse_small"], key
        else:
            assert s["fuse_small"] == (name != "tall"), key
            assert (s["search"] in (gen.SEARCH_HIST3, gen.SEARCH_HIST3_FIN)) == (name != "thin"), key
        loop = name == "thin" and not s["exhaustive"] and 2 <= bits <= 5 and 2 <= na <= TL_MAX_CAND
        assert s["try_thin_loop"] == int(loop), key
