"""CPU checks of the ALS contraction checker (oracle/als_bound.py).

The element-wise bounds |F - F64| <= (n_F + 4) 2^-24 BF and |G - G64| <= c_G 2^-24 BG must
accept an honest float32 numpy evaluation of every case of the table, in every mode, and
reject three local faults of the kinds a tiled MTTKRP kernel can have:

  drop_k_step   one 16-wide K-step missing from the bottom-right element;
  swap_kr_pair  the Khatri-Rao index pair (k / K2, k % K2) swapped at one k of that element;
  zero_row      the last valid row's contribution missing from the mode-2 row reduction
                (one column of F).

A kernel with such a fault runs every mode of a case, so per case and fault the test takes
the modes in which the fault exists, prints each, and asks the most exposed one to be at least
10 x outside the bound. What the bound cannot do is printed too: it is the worst case of n_F
roundings on n_F terms, so it grows as n_F^2 while one term or one K-step's 16 terms do not.
For standard normal inputs it overtakes a single term near n_F = 3000: the swapped pair in
mode 0 of (9,64,64) (n_F = 4096) is 0.37 of the bound, the same fault in the case's n_F = 576
modes 29 and 53 x outside. The table therefore reaches every form at a short reduction too.

The largest case (LARGE, a 128 x 64 x 9 layer whose output channels carry scales over four
decades, as trained conv layers do) shows what the whole-matrix 1e-5 relative Frobenius norm
cannot see: the same faults in the smallest channel leave it far below 1e-5 and are hundreds of
times outside the element's own bound. Every case prints the old number beside the new one.
"""
import functools

import numpy as np
import pytest

from oracle import als_bound as ab

TOL = 1e-5
LARGE = ((128, 64, 9), 134)


@functools.lru_cache(maxsize=None)
def _inputs(dims, R):
    if (dims, R) != LARGE:
        return ab.case_inputs(dims, R)
    g = np.random.default_rng(20)
    fs = [g.standard_normal((n, R), dtype=np.float32) for n in dims]
    scale = (10.0 ** (-4.0 * np.arange(dims[0]) / (dims[0] - 1))).astype(np.float32)
    W = g.standard_normal(dims, dtype=np.float32) * scale[:, None, None]
    return W, fs


def _operands32(W, fs, mode):
    """float32 (unfolding M x K, Khatri-Rao K x R, K2) in the k order of the unfolding."""
    o = ab.others(W.ndim, mode)
    unf = np.ascontiguousarray(np.moveaxis(W, mode, 0).reshape(W.shape[mode], -1))
    if len(o) == 1:
        return unf, fs[o[0]], 1
    kr = (fs[o[0]][:, None, :] * fs[o[1]][None, :, :]).reshape(-1, fs[0].shape[1])
    return unf, kr, W.shape[o[1]]


@functools.lru_cache(maxsize=None)
def _case(dims, R, mode):
    W, fs = _inputs(dims, R)
    unf, kr, _ = _operands32(W, fs, mode)
    F = (unf @ kr).astype(np.float32)
    G = np.ones((R, R), np.float32)
    for d in ab.others(len(dims), mode):
        G = (G * (fs[d].T @ fs[d])).astype(np.float32)
    return F, G, ab.reference(W, fs, mode)


def _drop_k_step(dims, R, mode, F):
    W, fs = _inputs(dims, R)
    unf, kr, _ = _operands32(W, fs, mode)
    K = unf.shape[1]
    if K < 16:
        return None
    k0 = (K // 16 - 1) * 16
    out = F.copy()
    out[-1, -1] -= np.float32(unf[-1, k0:k0 + 16] @ kr[k0:k0 + 16, -1])
    return out


def _swap_kr_pair(dims, R, mode, F):
    """KR[k] = X[k / K2] Y[k % K2] read as X[k % K2] Y[k / K2] at the last k where that is
    in range and another pair."""
    W, fs = _inputs(dims, R)
    if len(dims) == 2:
        return None
    unf, kr, K2 = _operands32(W, fs, mode)
    o = ab.others(3, mode)
    X, Y = fs[o[0]], fs[o[1]]
    ks = [k for k in range(unf.shape[1]) if k // K2 != k % K2 and k % K2 < X.shape[0] and k // K2 < Y.shape[0]]
    if not ks:
        return None
    k = ks[-1]
    out = F.copy()
    out[-1, -1] += unf[-1, k] * (X[k % K2, -1] * Y[k // K2, -1] - kr[k, -1])
    return out


def _zero_row(dims, R, mode, F):
    """Mode 2: F[s, r] = sum_i A[i, r] (sum_j W[i, j, s] B[j, r]) without i = I - 1, in the last column."""
    W, fs = _inputs(dims, R)
    if len(dims) == 2 or mode != 2 or dims[0] < 2:
        return None
    out = F.copy()
    out[:, -1] -= fs[0][-1, -1] * (W[-1].T @ fs[1][:, -1])
    return out


MUTATIONS = [_drop_k_step, _swap_kr_pair, _zero_row]
ALL = sorted({(c["dims"], c["R"]) for c in ab.CASES}) + [LARGE]


@pytest.mark.parametrize("dims,R", ALL, ids=lambda v: str(v).replace(" ", ""))
def test_bound_accepts_float32_evaluation(dims, R):
    for mode in range(len(dims)):
        F, G, (G64, F64, BG, BF) = _case(dims, R, mode)
        rf, rg = ab.worst_ratio(F, F64, BF), ab.worst_ratio(G, G64, BG)
        cf, cg = ab.f_constant(dims, mode), ab.g_constant(dims, mode)
        print(f"{dims} R={R} mode {mode}: F worst err / (2^-24 BF) = {rf:.3f} of c = {cf:.0f}, "
              f"G {rg:.3f} of c = {cg:.0f}; rel-Frobenius F {ab.rel_frobenius(F, F64):.2e}")
        assert rf <= cf and rg <= cg
        # float64 rounded once is well inside
        assert ab.worst_ratio(F64.astype(np.float32), F64, BF) <= 1.0
        assert ab.worst_ratio(G64.astype(np.float32), G64, BG) <= 1.0


@pytest.mark.parametrize("mutate", MUTATIONS, ids=lambda f: f.__name__.strip("_"))
def test_bound_rejects_local_faults(mutate):
    applied = 0
    for dims, R in ALL[:-1]:   # LARGE has its own test
        best = None
        for mode in range(len(dims)):
            F, _, (_, F64, _, BF) = _case(dims, R, mode)
            bad = mutate(dims, R, mode, F)
            if bad is None:   # the fault does not exist at this shape (K < 16, 2-way, not mode 2)
                continue
            c = ab.f_constant(dims, mode)
            ratio, frob = ab.worst_ratio(bad, F64, BF), ab.rel_frobenius(bad, F64)
            print(f"{dims} R={R} mode {mode} {mutate.__name__}: worst err / (2^-24 BF) = {ratio:.3g} = "
                  f"{ratio / c:.3g} x c = {c:.0f}; rel-Frobenius {frob:.2e} = {frob / TOL:.3g} x the 1e-5 threshold")
            assert int(np.sum(bad != F)) <= F.shape[0]   # a local fault: one element or one column
            best = max(best or 0.0, ratio / c)
        if best is not None:
            applied += 1
            assert best >= 10, (dims, R, best)
    assert applied >= 10


def test_frobenius_is_blind_on_the_largest_case():
    """LARGE, mode 0: the bottom-right element belongs to the smallest channel. A dropped K-step
    and a swapped Khatri-Rao pair there pass the 1e-5 relative Frobenius norm and are far more
    than 10 x outside the element's bound."""
    dims, R = LARGE
    assert np.prod(dims) > max(np.prod(c["dims"]) for c in ab.CASES)
    F, _, (_, F64, _, BF) = _case(dims, R, 0)
    c = ab.f_constant(dims, 0)
    assert ab.rel_frobenius(F, F64) < TOL and ab.worst_ratio(F, F64, BF) <= c
    for mutate in (_drop_k_step, _swap_kr_pair):
        bad = mutate(dims, R, 0, F)
        ratio, frob = ab.worst_ratio(bad, F64, BF), ab.rel_frobenius(bad, F64)
        print(f"{mutate.__name__}: rel-Frobenius {frob:.2e} (passes 1e-5), worst err / (2^-24 BF) = {ratio:.3g} "
              f"= {ratio / c:.3g} x c")
        assert frob < TOL
        assert ratio > 10 * c


def test_bound_rejects_nonfinite_zero_bound_and_shape():
    dims, R = (12, 32, 9), 33
    F, G, (G64, F64, BG, BF) = _case(dims, R, 1)
    bad = F.copy()
    bad[3, 5] = np.nan
    assert ab.worst_ratio(bad, F64, BF) == float("inf")
    bad[3, 5] = np.inf
    assert ab.worst_ratio(bad, F64, BF) == float("inf")
    Bz = BF.copy()
    Bz[0, 0] = 0.0
    assert ab.worst_ratio(F, F64, Bz) == float("inf")
    assert ab.worst_ratio(F64.copy(), F64, Bz) <= 1.0        # no error where the bound is 0: fine
    assert ab.worst_ratio(F[:-1], F64, BF) == float("inf")
    assert ab.worst_ratio(G, G64, BG) <= ab.g_constant(dims, 1)


def test_reference_matches_the_plain_einsum():
    """The tensordot route of the reference against the (I, J, R) einsum it avoids."""
    for dims, R in [((12, 32, 9), 33), ((7, 150, 7), 65), ((1, 17, 3), 40)]:
        W, fs = ab.case_inputs(dims, R)
        W64, (A, B, C) = W.astype(np.float64), [f.astype(np.float64) for f in fs]
        want = [np.einsum("ijk,jr,kr->ir", W64, B, C), np.einsum("ijk,ir,kr->jr", W64, A, C),
                np.einsum("ijk,ir,jr->kr", W64, A, B)]
        for mode in range(3):
            G64, F64, BG, BF = ab.case_reference(dims, R, mode)
            assert np.allclose(F64, want[mode], rtol=1e-12, atol=1e-12)
            assert np.all(BF >= np.abs(F64)) and np.all(BG >= np.abs(G64) * (1 - 1e-12))
    W, fs = ab.case_inputs((5, 1030), 3)
    G64, F64, _, _ = ab.case_reference((5, 1030), 3, 1)
    assert np.allclose(F64, W.astype(np.float64).T @ fs[0].astype(np.float64), rtol=1e-12, atol=1e-12)
    assert np.allclose(G64, fs[0].astype(np.float64).T @ fs[0].astype(np.float64), rtol=1e-12, atol=1e-12)
