"""The MSE-minmax search at every (bits, num_attempts) cell that fixes its device form
(csrc/admm_plan.hip: search_form, schedule_run; csrc/mse_search.hip: launch_mse_*), against
the CPU oracle, which tests/test_oracle_golden.py pins to the reference at these cells (F13).
Run on an MI355X with `pytest -m gpu`. The forms, by cell (tests/test_search_form_host.py
restates the rule):

  exhaustive sweep            7 and 8 bits; 1100 candidates
  per-level stage 1           6 bits; 1 candidate; 196 / 201 candidates at 4 and 5 bits (a tie
                              group above 4)
  merged-threshold stage 1    everything else at 1..5 bits, its finalize fused or separate,
                              the thin factors in k_mse_small_admm<QMAX, G>
  persistent thin loop        an all-thin batch at 2..5 bits and 2..256 candidates

Shapes are the smallest that reach each kernel (ld = roundup(R, 32), 4096-element units of
whole rows): tall (40, 134) has 2 units and (64, 278) 5, the thin factors (9, 134),
(16, 278), (9, 1141), (12, 1141) and (16, 1141) give k_mse_small_admm's G = 1, 2, 3, 4, 6.
Four iterations per run, inputs near unit scale. Every comparison is bit for bit.
"""
import functools

import numpy as np
import pytest

import golden_cases as gc
from conftest import gpu_available
from oracle import quant_oracle as qo

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE = "tensor_mseminmax_symmetric"
ITERS = 4
GRID = gc.f13_grid()
BATCHES = {
    "mixed": [(40, 134), (64, 278), (9, 134)],     # G = 1
    "mixed6": [(40, 134), (16, 1141)],             # G = 6
    "thin": [(9, 134), (9, 40)],                   # every factor thin: the persistent loop where it runs
    "g2": [(40, 134), (16, 278)], "g3": [(40, 134), (9, 1141)], "g4": [(40, 134), (12, 1141)],
}


def _bits(a):
    return gc.canonical_sha(np.asarray(a, np.float32))


@functools.lru_cache(maxsize=None)
def _gram(R):
    """SPD, as tests/test_gpu_search_setup.py builds it."""
    rng = np.random.default_rng(7000 + R)
    B = rng.standard_normal((R, 2 * R)).astype(np.float32) / np.float32(np.sqrt(2 * R))
    return (B @ B.T + 0.5 * np.eye(R)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _batch(name):
    """[(H0, U0, F, G)] of a batch on the device (read only: every run clones U), and U0 on the host."""
    import torch
    dev = torch.device("cuda:0")
    out, u0 = [], []
    for k, (I, R) in enumerate(BATCHES[name]):
        rng = np.random.default_rng(100000 * k + 1000 * I + R)
        F = rng.standard_normal((I, R)).astype(np.float32)
        H0 = (rng.standard_normal((I, R)) * 0.1).astype(np.float32)
        U0 = (rng.standard_normal((I, R)) * 0.01).astype(np.float32)
        out.append(tuple(torch.from_numpy(a).to(dev) for a in (H0, U0, F, _gram(R))))
        u0.append(U0)
    return out, u0


def _run(name, bits, na, iters=ITERS, qscheme=MSE):
    """One call: [(H, U, H_T, X)] on the host and info."""
    from admmq import admm_iteration_batched
    ps = [(H0, U0.clone(), F, G) for H0, U0, F, G in _batch(name)[0]]
    Hs, dbg, info = admm_iteration_batched(ps, iters + 1, 0.0, bits, qscheme, num_attempts=na, debug_outputs=True,
                                           return_info=True)
    info = info.cpu().numpy()
    assert (info[:, 3] == 0).all() and (info[:, 4] == 0).all(), info     # no internal fault, no re-run
    assert (info[:, 0] == iters).all() and (info[:, 2] == 0).all(), info
    return [tuple(a.cpu().numpy() for a in (H, p[1], HT, X)) for H, p, (HT, X) in zip(Hs, ps, dbg)]


def _candidate(H, X, bits, na):
    """The candidate whose grid step H lies on (for the failure message)."""
    _, s = gc.grid_levels(H)
    mx = np.float32(np.abs(X).max())
    scales = (np.float32(2.0) * qo.candidate_grid(mx, na)) / np.float32(2 ** bits - 1)
    hit = np.flatnonzero(scales.astype(np.float32) == s)
    return int(hit[0]) if hit.size else None


def _check_batch(name, bits, na, forms):
    """The default run against the oracle and the one-step dual update, then every other
    form against the default run."""
    from admmq import _lib
    repairs0 = _lib.fault_repairs()
    ref = _run(name, bits, na)
    for p, (H, _, _, X) in enumerate(ref):
        Hq, inf = qo.quantize_tensor_mse(X, bits, na, return_info=True)
        assert _bits(H) == _bits(Hq), (f"projection: bits={bits} na={na} {name}[{p}] {BATCHES[name][p]}: the oracle "
                                       f"chose candidate {inf['index']}, the kernel {_candidate(H, X, bits, na)}")
    for p, ((H, U, HT, X), U0) in enumerate(zip(_run(name, bits, na, iters=1), _batch(name)[1])):
        assert _bits(X) == _bits((HT - U0).astype(np.float32)), (name, p, "X")
        Hq = qo.quantize_tensor_mse(X, bits, na)
        assert _bits(H) == _bits(Hq), (name, p, "one-step projection")
        assert _bits(U) == _bits((U0 + (Hq - HT).astype(np.float32)).astype(np.float32)), (name, p, "dual update")
    for form, cm in forms:
        with cm():
            other = _run(name, bits, na)
        for p, (a, b) in enumerate(zip(ref, other)):
            if _bits(a[3]) != _bits(b[3]):   # an earlier iteration differed: which form left the oracle's path?
                assert _bits(b[0]) == _bits(qo.quantize_tensor_mse(b[3], bits, na)), (form, name, p, "projection")
            assert _bits(a[0]) == _bits(b[0]), (form, name, p, "H")
            assert _bits(a[1]) == _bits(b[1]), (form, name, p, "U")
    assert _lib.fault_repairs() == repairs0


def _forms(thin=False):
    import contextlib
    from admmq import _lib
    forms = [("second run", contextlib.nullcontext), ("separate finalize", lambda: _lib.fused_finalize(False)),
             ("per-level stage 1", lambda: _lib.stage1_form("legacy")), ("exhaustive", _lib.exhaustive_search)]
    if thin:
        forms.append(("per-iteration launches", lambda: _lib.thin_loop(False)))
    return forms


@pytest.mark.parametrize("bits,na", GRID)
def test_mixed_batches_equal_oracle(bits, na):
    """Tall and thin factors in one call: the per-iteration path, the fused finalize and
    k_mse_small_admm (G = 1 and 6) where the cell takes the merged stage 1."""
    _check_batch("mixed", bits, na, _forms())
    _check_batch("mixed6", bits, na, _forms())


@pytest.mark.parametrize("bits,na", GRID)
def test_all_thin_batch_equals_oracle(bits, na):
    """Every factor thin: the persistent loop at 2..5 bits and up to 256 candidates, the
    per-iteration launches in every other cell (1, 6, 7 and 8 bits, 1100 candidates)."""
    _check_batch("thin", bits, na, _forms(thin=True))


@pytest.mark.parametrize("na", gc.F13_ATTEMPTS)
@pytest.mark.parametrize("name", ["g2", "g3", "g4"])
def test_small_job_groups_equal_oracle(name, na):
    """k_mse_small_admm's G = 2, 3 and 4 (3 bits)."""
    _check_batch(name, 3, na, _forms())


@functools.lru_cache(maxsize=None)
def _f13():
    """{(bits, na): [(input on the device, reference SHA)]} of the three F13 inputs."""
    import torch
    dev = torch.device("cuda:0")
    xs, out = {}, {}
    for case in gc.f13_reference():
        if case["kind"] not in xs:
            xs[case["kind"]] = torch.from_numpy(gc.f13_input(case)).to(dev)
        out.setdefault((case["bits"], case["num_attempts"]), []).append((xs[case["kind"]], case["sha"], case["id"]))
    return out


@pytest.mark.parametrize("bits,na", GRID)
def test_standalone_quantizer_equals_reference(bits, na):
    """quantize_batched of the three F13 inputs (one call) against the reference's own
    outputs, in the cell's default form, the per-level stage 1 and the exhaustive sweep."""
    import contextlib
    from admmq import _lib, quantize_batched
    cases = _f13()[(bits, na)]
    assert len(cases) == 3
    for form, cm in (("default", contextlib.nullcontext), ("per-level stage 1", lambda: _lib.stage1_form("legacy")),
                     ("exhaustive", _lib.exhaustive_search)):
        with cm():
            ys = quantize_batched([x for x, _, _ in cases], bits, MSE, num_attempts=na)
        for y, (_, sha, cid) in zip(ys, cases):
            assert _bits(y.cpu().numpy()) == sha, (form, cid)


@functools.lru_cache(maxsize=None)
def _negative_inputs():
    """Twelve small tensors without a positive element, on the host and on the device."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(606)
    xs = [(-np.abs(rng.standard_normal(s)) * 0.3).astype(np.float32) for s in [(9, 40), (16, 70), (25, 134)] * 4]
    return xs, [torch.from_numpy(x).to(dev) for x in xs]


@pytest.mark.parametrize("na", [n for n in gc.F13_ATTEMPTS if n > 1])
@pytest.mark.parametrize("bits", [5, 6])
def test_top_level_of_negative_elements(bits, na):
    """Level QMAX = 2^(bits-1) is reached by negative elements only, by every one of them
    above 0.2 max|x|; in the per-level stage 1 (6 bits, and the forced legacy form at 5) it
    is bit QMAX of hist_insert_elem's slow-path mask, which a 32-bit mask lost at QMAX = 32:
    the level's sums then missed the elements whose breakpoint estimate was off, and the
    selection could drop the argmin. All-negative tensors make every element a candidate for
    that path; against the oracle, in the default and the per-level form."""
    import contextlib
    from admmq import _lib, quantize_batched
    xs, xd = _negative_inputs()
    want = [_bits(qo.quantize_tensor_mse(x, bits, na)) for x in xs]
    for form, cm in (("default", contextlib.nullcontext), ("per-level stage 1", lambda: _lib.stage1_form("legacy"))):
        with cm():
            ys = quantize_batched(xd, bits, MSE, num_attempts=na)
        assert [_bits(y.cpu().numpy()) for y in ys] == want, form


# (tensor_minmax at 1 bit is sign(x) - 1, no grid of the scheme: left to the quantizer's own KATs)
@pytest.mark.parametrize("qscheme,bits", [(q, b) for q in ("tensor_minmax", "tensor_symmetric", "tensor_affine")
                                          for b in (1, 2, 3, 6, 8) if (q, b) != ("tensor_minmax", 1)])
def test_other_schemes_one_step(qscheme, bits):
    """k_finalize_admm's other schemes at the widths no other test runs them at: one step,
    the projection and the dual update against the oracle given the kernel's own H_T."""
    for name in ("mixed", "thin"):
        for p, ((H, U, HT, X), U0) in enumerate(zip(_run(name, bits, 200, iters=1, qscheme=qscheme), _batch(name)[1])):
            assert _bits(X) == _bits((HT - U0).astype(np.float32)), (name, p, "X")
            Hq = qo.quantize_tensor(X, bits, qscheme)
            assert _bits(H) == _bits(Hq), (name, p, "projection")
            assert _bits(U) == _bits((U0 + (Hq - HT).astype(np.float32)).astype(np.float32)), (name, p, "dual update")
