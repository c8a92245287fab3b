"""The fused search's stage-1 table setup (k_mse_hist3: h3_setup, h3_insert_n): the buckets
zeroed early with 16-byte stores, e / n by a multiply, the two-member tie groups ordered
without the sort loops, and +inf entries after the sorted thresholds in place of the probes'
clamps and bounds. None of this may change a bit. Run on an MI355X with `pytest -m gpu`.

Each batch holds factors of one rank with row counts that give jobs of 1, 2, 3 and >= 8
search blocks (4096-element whole-row units), plus an all-zero factor (degenerate max|x|),
and factors scaled so that max|x| is about 2^-101 and 2^101 (outside the range the host
order is used for: those jobs rank the thresholds by counting, the +inf entries still
behind them). 2, 4 and 5 bits (5 bits at 200 candidates has 66 tie groups, 4 bits 5, the
others none) and 3 and 200 candidates; eight iterations per run. Compared bit for bit: the
fused launch (run twice back to back, in the same workspace memory), the separate finalize
launch (the kernel's other form) and the exhaustive search, which builds no table; the last
iteration's projection against oracle/quant_oracle.py. The selection is compared through
the projection's grid step (the selected candidate fixes it).

The factor near 2^101 is compared among the two-stage forms only: the canonical SSE squares
float32 residuals of about 2^101 / (2^bits - 1), which overflow float32 above 2^64, so every
candidate's canonical SSE is inf and neither the exhaustive search nor the oracle (a
float -> uint64 cast of inf) defines an answer there."""
import functools

import numpy as np
import pytest

import golden_cases as gc
from conftest import gpu_available
from oracle import quant_oracle as qo

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE = "tensor_mseminmax_symmetric"
ITERS = 8
# (I, R) of the issue, and the extra row counts of the same rank: with ld = roundup(R, 32)
# and 4096-element units of whole rows, R = 134 has 25 rows per unit, R = 278 has 14,
# R = 1141 has 3
BATCHES = {
    (64, 134): [20, 40, 64, 230],        # 1, 2, 3, 10 blocks
    (128, 278): [17, 28, 42, 128],       # 2, 2, 3, 10 blocks (<= 16 rows would be a thin factor)
    (40, 1141): [17, 20, 24, 40],        # 6, 7, 8, 14 blocks (a row fills over a quarter of a unit)
}


def _bits(a):
    return gc.canonical_sha(np.asarray(a, np.float32))


@functools.lru_cache(maxsize=None)
def _batch(I, R):
    """[(H0, U0, F, G, kind)] of one batch (host arrays, shared by every case of the batch)."""
    rng = np.random.default_rng(1000 * I + R)
    B = rng.standard_normal((R, 2 * R)).astype(np.float32) / np.float32(np.sqrt(2 * R))
    G = (B @ B.T + 0.5 * np.eye(R)).astype(np.float32)
    out = []
    for rows in BATCHES[(I, R)]:
        F = rng.standard_normal((rows, R)).astype(np.float32)
        H0 = (rng.standard_normal((rows, R)) * 0.1).astype(np.float32)
        U0 = (rng.standard_normal((rows, R)) * 0.01).astype(np.float32)
        out.append((H0, U0, F, G, "plain"))
    z = np.zeros((I, R), np.float32)
    out.append((z, z, z, G, "zero"))
    # max|H_T - U| of these inputs is about 2^2 (|F| up to ~4, G near the identity scale): the
    # power-of-two factors put it near 2^-101 and 2^101 (the test checks the last iteration's)
    F = rng.standard_normal((I, R)).astype(np.float32)
    H0 = (rng.standard_normal((I, R)) * 0.1).astype(np.float32)
    U0 = (rng.standard_normal((I, R)) * 0.01).astype(np.float32)
    for kind, e in (("tiny", -103), ("huge", 99)):
        s = np.float32(2.0 ** e)
        out.append((H0 * s, U0 * s, F * s, G, kind))
    return out


def _run(torch, dev, probs, bits, na, **kw):
    from admmq import admm_iteration_batched
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ps = [(t(H0), t(U0), t(F), t(G)) for H0, U0, F, G, _ in probs]
    Hs, dbg, info = admm_iteration_batched(ps, ITERS + 1, 0.0, bits, MSE, num_attempts=na, debug_outputs=True,
                                           return_info=True, **kw)
    info = info.cpu().numpy()
    return [(H.cpu().numpy(), p[1].cpu().numpy(), X.cpu().numpy()) for H, p, (_, X) in zip(Hs, ps, dbg)], info


def _step(H):
    a = np.abs(H[np.isfinite(H)])
    a = a[a > 0]
    return float(a.min()) if a.size else 0.0


def _case(I, R, bits, na):
    import torch
    from admmq import _lib
    dev = torch.device("cuda:0")
    probs = _batch(I, R)
    repairs0 = _lib.fault_repairs()

    on1, i1 = _run(torch, dev, probs, bits, na)
    on2, i2 = _run(torch, dev, probs, bits, na)          # back to back: the same workspace memory again
    with _lib.fused_finalize(False):
        sep, i4 = _run(torch, dev, probs, bits, na)
    with _lib.exhaustive_search():
        exh, i5 = _run(torch, dev, probs, bits, na)
    kinds = [p[4] for p in probs]

    for info in (i1, i2, i4, i5):
        assert (info[:, 3] == 0).all(), info             # no internal fault (bounded waits)
        assert (info[:, 0] == ITERS).all(), info
    assert (i1[:, 4] == 0).all() and (i2[:, 4] == 0).all() and _lib.fault_repairs() == repairs0
    for name, other in (("second run", on2), ("separate finalize", sep), ("exhaustive", exh)):
        for p, (a, b) in enumerate(zip(on1, other)):
            if name == "exhaustive" and kinds[p] == "huge":
                continue                                  # (no defined answer: the module docstring)
            assert _bits(a[0]) == _bits(b[0]), (name, p, kinds[p], "H")
            assert _bits(a[1]) == _bits(b[1]), (name, p, kinds[p], "U")
            assert _step(a[0]) == _step(b[0]), (name, p, kinds[p], "selection")

    for (H, _, X), kind in zip(on1, kinds):
        mx = float(np.abs(X).max())
        if kind == "zero":   # degenerate from the first iteration on: its projection is NaN, and so is all after it
            assert np.isnan(X).all() and np.isnan(H).all()
        elif kind == "tiny":
            assert 0.0 < mx < 2.0 ** -100, mx
        elif kind == "huge":
            assert 2.0 ** 100 < mx < np.inf, mx
            continue                                      # (no defined answer: the module docstring)
        Hq = qo.quantize_tensor_mse(X, bits, na)
        assert _bits(H) == _bits(Hq), kind


@pytest.mark.parametrize("na", [3, 200])
@pytest.mark.parametrize("bits", [2, 4, 5])
@pytest.mark.parametrize("I,R", sorted(BATCHES))
def test_search_setup_same_bits(I, R, bits, na):
    _case(I, R, bits, na)
