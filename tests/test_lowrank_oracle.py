"""The numpy restatement of scripts/factorize_lowrank.py (oracle/lowrank_oracle.py) against
the reference's own outputs (tests/golden/f6_lowrank.npz, made by gen_golden.py --only f6)."""
import os
from functools import partial

import numpy as np
import pytest

from oracle import lowrank_oracle as lo
from oracle import quant_oracle as qo

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def f6():
    return np.load(os.path.join(GOLDEN, "f6_lowrank.npz"))


def _rel(a, b):
    return float(np.linalg.norm(np.float64(a) - np.float64(b)) / np.linalg.norm(np.float64(b)))


@pytest.mark.parametrize("qs", ["tensor_minmax", "tensor_mseminmax_symmetric"])
@pytest.mark.parametrize("mi", [2, 3, 50])
def test_quant_side_bit_exact(f6, qs, mi):
    """Elementwise float32 updates + the bit-exact quantizer: identical to the reference."""
    qf = partial(qo.quantize_tensor, bits=4, qscheme=qs)
    H, U, _ = lo.admm_iteration(f6["Wq0"], np.zeros_like(f6["Wq0"]), f6["W"], f6["Wr0"], qf, 1.0, mi)
    assert np.array_equal(H.view(np.uint32), f6[f"{qs}_q_it{mi}_H"].view(np.uint32))
    assert np.array_equal(U.view(np.uint32), f6[f"{qs}_q_it{mi}_U"].view(np.uint32))


@pytest.mark.parametrize("mi", [2, 3])
def test_rank_side(f6, mi):
    """SVD truncation (numpy LAPACK vs torch's): within 1e-5 rel-Frobenius."""
    pf = partial(lo.project_rank, rank=4)
    H, U, _ = lo.admm_iteration(f6["Wr0"], np.zeros_like(f6["Wr0"]), f6["W"], f6["Wq0"], pf, 1.0, mi)
    assert _rel(H, f6[f"r_it{mi}_H"]) < 1e-5
    assert _rel(U, f6[f"r_it{mi}_U"]) < 1e-5
    assert np.linalg.matrix_rank(H.astype(np.float64), tol=1e-4 * np.linalg.norm(H)) <= 4


# (shape, rho, eps, the iteration the oracle breaks at); tests/test_gpu_lowrank.py runs the same.
# At rho = 1 the loop's fixed point makes |H - H_prev| and |H - H_| agree to three digits
# near the break, so a post kernel that formed s from H_ instead of H_prev breaks at the
# same iteration there; at rho = 2 it breaks two iterations late (13 instead of 11).
BREAK_CASES = [((7, 11), 1.0, 0.02, 8), ((33, 31), 1.0, 0.02, 11), ((96, 64), 1.0, 0.02, 12),
               ((33, 31), 2.0, 0.005, 11)]


@pytest.mark.parametrize("shape,rho,eps,k", BREAK_CASES)
def test_break_cases_sit_off_the_threshold(shape, rho, eps, k):
    """The inputs of the GPU break-at-iteration-k test (lo.break_case, U = 0, max_iter = 40,
    the round-to-quarters projection): the oracle breaks at iteration k > 1, and at every
    iteration the ratio that decides the test, max(r, s), is at least 25 % away from eps.
    The device sums its residuals in another order than numpy (both in float64, relative
    difference ~1e-13), so its decisions are the oracle's at every iteration."""
    W, H2, H0 = lo.break_case(shape)
    hist = []
    _, _, it = lo.admm_iteration(H0, np.zeros_like(H0), W, H2, lo.proj_quarter, rho, 40, eps, history=hist)
    assert it == k == len(hist) and 1 < k < 39
    for j, (r, s) in enumerate(hist):
        m = max(r, s)
        assert np.isfinite(m)
        assert m >= 1.25 * eps or m <= eps / 1.25, (j + 1, r, s)
        assert (m < eps) == (j + 1 == k)


def test_history_is_optional():
    """The (r, s) history does not change what the oracle returns."""
    W, H2, H0 = lo.break_case((7, 11))
    a = lo.admm_iteration(H0, np.zeros_like(H0), W, H2, lo.proj_quarter, 1.0, 40, 0.02)
    hist = []
    b = lo.admm_iteration(H0, np.zeros_like(H0), W, H2, lo.proj_quarter, 1.0, 40, 0.02, history=hist)
    assert a[2] == b[2] == len(hist)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
