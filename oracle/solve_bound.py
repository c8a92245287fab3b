"""ORACLE - test infrastructure only. The element-wise check of the ADMM solve step
H_T = P M, P = F + rho (H + U), M = (G + rho I)^-1 (source/admm.py:53-57), and the fixed
cases of the stop-rule tests (source/admm.py:62-65). Shared by tests/test_solve_bound_host.py
(CPU) and tests/test_gpu_solve_forms.py / tests/test_gpu_stop_rule.py (GPU).

The bound. With u = 2^-24 (float32 unit roundoff) and M the float32 inverse the device
itself uses, the float64 product want = P64 M of the float32 inputs and

    B = (|F| + |rho| (|H| + |U|)) |M|          (element-wise absolute values),

any float32 evaluation of the step satisfies, per element,

    |H_T[i,j] - want[i,j]| <= (R + 4) u B[i,j].

Derivation: forming P = F + rho (H + U) in float32 rounds at most three times (the sum, the
product, the sum; two with an FMA), each relative to a quantity no larger than
|F| + |rho| (|H| + |U|): 3 u. The dot product of R terms, in ANY order and any grouping -
one FMA chain, an MFMA K order, partial chains summed in piece order, a K-split over
workgroups, the thin solve's class chains - passes every product through at most R
roundings (R - 1 additions and the product's own, fewer with FMAs), so it is within
R u sum_k |P_ik| |M_kj| to first order; padded K entries are exact zeros and add nothing.
One unit is spare for the second-order terms ((R + 3)^2 u^2 / 2 < u up to R = 5000).
Hence c = R + 3 + 1 = R + 4. Nothing in it is measured.

What the whole-matrix 1e-5 relative Frobenius norm cannot see and this bound does: one
dropped K-step of a single element is an error of about sqrt(32 / R) of that element's
B, thousands of times (R + 4) u; tests/test_solve_bound_host.py shows it.
"""
from __future__ import annotations

import numpy as np

from . import admm_oracle as ao

U32 = 2.0 ** -24
MSE = "tensor_mseminmax_symmetric"


def device_a64(G: np.ndarray, rho: np.float32) -> np.ndarray:
    """float64 of the float32 values the device's fill kernel forms: g + rho on the diagonal
    (a float32 sum), g elsewhere."""
    return ao.shifted_gram(np.asarray(G, np.float32), np.float32(rho)).astype(np.float64)


def reference(H, U, F, rho, M):
    """(want, B) in float64 for one solve step from the float32 inputs and the inverse M
    (R x R, the device's own float32 values)."""
    H, U, F = (np.asarray(a, np.float32).astype(np.float64) for a in (H, U, F))
    M = np.asarray(M, np.float64)
    r = float(np.float32(rho))
    want = (F + r * (H + U)) @ M
    B = (np.abs(F) + abs(r) * (np.abs(H) + np.abs(U))) @ np.abs(M)
    return want, B


def worst_ratio(HT, want, B) -> float:
    """max over the elements of |H_T - want| / (u B); inf where B = 0 and the error is not."""
    err = np.abs(np.asarray(HT, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(B > 0, err / (U32 * B), np.where(err > 0, np.inf, 0.0))
    if not np.all(np.isfinite(np.asarray(HT))):
        return float("inf")
    return float(q.max())


def fp32_constant(R: int) -> int:
    """c of the derived bound for the float32 forms."""
    return R + 4


def rel_frobenius(a, b) -> float:
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def solve_problem(I: int, R: int):
    """(H0, U0, F, G) float32 of the solve-form cases, fixed by the shape: G = B B^T + I / 2
    with B (R, R + 64) scaled to unit row variance, F and H0 standard normal, U0 a tenth of
    that (large enough that a dropped U moves H_T far outside the bound)."""
    rng = np.random.default_rng(100003 * I + R)
    Bm = rng.standard_normal((R, R + 64), dtype=np.float32) / np.float32(np.sqrt(R + 64))
    G = (Bm @ Bm.T + np.float32(0.5) * np.eye(R, dtype=np.float32)).astype(np.float32)
    G = ((G + G.T) * np.float32(0.5)).astype(np.float32)
    H0 = rng.standard_normal((I, R), dtype=np.float32)
    U0 = (rng.standard_normal((I, R), dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    F = rng.standard_normal((I, R), dtype=np.float32)
    return H0, U0, F, G


# --------------------------------------------------------------------------------------
# The stop rule. G = B B^T + ridge I, U0 = 0 (as tests/test_gpu_launch_head.py); per batch
# one eps at which the reference stops the three problems at three distinct iterations, all
# <= 8, with the deciding max(r, s) of every iteration up to the stop at least 25 % away from
# eps - a condition on the inputs (found by a search over seeds and ridges on the CPU with
# this oracle), which tests/test_solve_bound_host.py asserts from the oracle's history.
STOP_MARGIN = 0.25
# name -> (qscheme, eps, [(I, R, seed, ridge)], [the reference's stop iteration])
STOP_BATCHES = {
    "thin": (MSE, 0.3017, [(9, 134, 5, 4.0), (16, 278, 3, 8.0), (9, 40, 2, 0.5)], [6, 7, 8]),
    "mixed": (MSE, 0.2628, [(9, 134, 5, 4.0), (40, 70, 3, 0.5), (65, 129, 4, 4.0)], [6, 8, 7]),
    "minmax": ("tensor_minmax", 0.3159, [(9, 134, 4, 1.0), (40, 70, 6, 4.0), (65, 129, 2, 2.0)], [8, 6, 7]),
    "symmetric": ("tensor_symmetric", 0.757, [(9, 134, 3, 0.25), (40, 70, 6, 2.0), (65, 129, 1, 0.5)], [6, 4, 5]),
    "affine": ("tensor_affine", 0.4564, [(9, 134, 7, 0.5), (40, 70, 6, 4.0), (65, 129, 7, 8.0)], [7, 5, 6]),
}
STOP_MAX_ITER = 12   # max_iter of the early-exit runs: every stop is at most 8


def stop_eps(name: str) -> float:
    """The batch's eps as the float32 the device receives."""
    return float(np.float32(STOP_BATCHES[name][1]))


def stop_problem(I, R, seed, ridge):
    rng = np.random.default_rng(seed)
    Bm = rng.standard_normal((R, 2 * R)) / np.sqrt(2 * R)
    G = (Bm @ Bm.T + ridge * np.eye(R)).astype(np.float32)
    F = rng.standard_normal((I, R)).astype(np.float32)
    H = (rng.standard_normal((I, R)) * 0.1).astype(np.float32)
    return H, F, G


def stop_history(name: str, k: int, max_iter: int = STOP_MAX_ITER):
    """(iterations the reference runs, [(r, s)] per iteration) of problem k of a batch."""
    scheme, _, specs, _ = STOP_BATCHES[name]
    H, F, G = stop_problem(*specs[k])
    hist = []
    _, _, info = ao.admm_iteration(H, np.zeros_like(H), F, G, max_iter, stop_eps(name), 4, scheme, return_info=True,
                                   history=hist)
    return info["iters"], hist


def stop_margin(hist, eps: float) -> float:
    """min over the iterations of |max(r, s) / eps - 1|."""
    return min(abs(max(r, s) / eps - 1.0) for r, s in hist)
