"""CPU checks of the solve-step checker (oracle/solve_bound.py) and of the stop-rule cases.

The element-wise bound |H_T - want| <= (R + 4) 2^-24 B must accept an honest float32 P M and
reject the faults the whole-matrix 1e-5 relative Frobenius norm was blind to (or nearly): a
K-step of 32 terms dropped from a single edge element, the last valid column replaced by its
neighbour, a K-split piece added twice to one row. Each case prints the old number beside
the new ratio.

The stop-rule cases (oracle.solve_bound.STOP_BATCHES) are conditions on the inputs: the
reference stops the three problems of a batch at three distinct iterations <= 8, and the
deciding max(r, s) of every iteration up to the stop is at least 25 % away from eps. They
are asserted here from the oracle's history, so the GPU tests' cases stay valid if the
oracle moves.
"""
import numpy as np
import pytest

from oracle import admm_oracle as ao
from oracle import solve_bound as sb

CASES = [(65, 129), (9, 1185)]


def _case(I, R):
    H0, U0, F, G = sb.solve_problem(I, R)
    rho = ao.rho_of(G)
    M = np.linalg.inv(sb.device_a64(G, rho)).astype(np.float32)
    P = (F + (rho * (H0 + U0).astype(np.float32)).astype(np.float32)).astype(np.float32)
    HT = (P @ M).astype(np.float32)
    want, B = sb.reference(H0, U0, F, rho, M)
    return P, M, HT, want, B


def _drop_k_step(P, M, HT):
    """The last whole 32-term K-step missing from the bottom-right valid element."""
    I, R = HT.shape
    k0 = (R // 32 - 1) * 32
    out = HT.copy()
    out[I - 1, R - 1] -= np.float32(P[I - 1, k0:k0 + 32] @ M[k0:k0 + 32, R - 1])
    return out


def _neighbour_column(P, M, HT):
    out = HT.copy()
    out[:, -1] = out[:, -2]
    return out


def _piece_twice(P, M, HT):
    """The first of three K pieces folded twice into the last row."""
    I, R = HT.shape
    k1 = (R + 31) // 32 // 3 * 32
    assert k1 >= 32
    out = HT.copy()
    out[I - 1, :] += (P[I - 1, :k1] @ M[:k1, :]).astype(np.float32)
    return out


@pytest.mark.parametrize("I,R", CASES)
def test_bound_accepts_float32_product(I, R):
    P, M, HT, want, B = _case(I, R)
    ratio = sb.worst_ratio(HT, want, B)
    print(f"({I},{R}) numpy float32 P @ M: worst err / (2^-24 B) = {ratio:.3f} of c = {sb.fp32_constant(R)}, "
          f"rel-Frobenius {sb.rel_frobenius(HT, want):.2e}")
    assert ratio <= sb.fp32_constant(R)
    # float64 rounded once is well inside
    assert sb.worst_ratio(want.astype(np.float32), want, B) <= 1.0


@pytest.mark.parametrize("mutate", [_drop_k_step, _neighbour_column, _piece_twice], ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("I,R", CASES)
def test_bound_rejects_local_faults(I, R, mutate):
    P, M, HT, want, B = _case(I, R)
    bad = mutate(P, M, HT)
    ratio = sb.worst_ratio(bad, want, B)
    frob = sb.rel_frobenius(bad, want)
    print(f"({I},{R}) {mutate.__name__}: worst err / (2^-24 B) = {ratio:.3g} against c = {sb.fp32_constant(R)}; "
          f"rel-Frobenius {frob:.2e} = {frob / 1e-5:.3g} x the 1e-5 threshold")
    assert ratio > sb.fp32_constant(R)
    assert int(np.sum(bad != HT)) <= max(HT.shape)   # a local fault: one element, one column or one row


def test_bound_rejects_nonfinite_and_zero_bound():
    P, M, HT, want, B = _case(65, 129)
    bad = HT.copy()
    bad[3, 5] = np.nan
    assert sb.worst_ratio(bad, want, B) == float("inf")
    Bz = B.copy()
    Bz[0, 0] = 0.0
    assert sb.worst_ratio(HT, want, Bz) == float("inf")


def test_history_is_optional_and_matches_the_stop():
    H, F, G = sb.stop_problem(9, 40, 2, 0.5)
    U = np.zeros_like(H)
    a = ao.admm_iteration(H, U, F, G, 6, 0.0, 4, sb.MSE)
    hist = []
    b = ao.admm_iteration(H, U, F, G, 6, 0.0, 4, sb.MSE, history=hist)
    assert len(a) == 2 and len(b) == 2 and len(hist) == 5
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert all(r >= 0 and s >= 0 for r, s in hist)


@pytest.mark.parametrize("name", list(sb.STOP_BATCHES))
def test_stop_cases_have_their_margin(name):
    scheme, _, specs, stops = sb.STOP_BATCHES[name]
    eps = sb.stop_eps(name)
    assert len(set(stops)) == 3 and max(stops) <= 8 and max(stops) < sb.STOP_MAX_ITER - 1
    for k, (spec, want) in enumerate(zip(specs, stops)):
        iters, hist = sb.stop_history(name, k)
        m = [max(r, s) for r, s in hist]
        margin = sb.stop_margin(hist, eps)
        print(f"{name} {scheme} eps {eps:.4f} {spec}: stops at {iters}, max(r, s) "
              f"{' '.join('%.3g' % v for v in m)}, margin {margin:.3f}")
        assert iters == want == len(hist)
        assert all(v >= eps for v in m[:-1]) and m[-1] < eps
        assert margin >= sb.STOP_MARGIN
