"""ORACLE - test infrastructure only. The element-wise check of the ALS-sweep contractions
(scripts/factorize.py:215-237, :276-287): for mode n of a layer W with factors A, B (, C)

    F = W_(n) KR(others)            (MTTKRP: the mode-n unfolding times the Khatri-Rao product)
    G = (X^T X) o (Y^T Y)           (Hadamard product of the other factors' Grams; 2-way: X^T X)

and the case table of tests/test_gpu_als_forms.py with the kernel form each case is there
for. Shared by tests/test_als_bound_host.py, tests/test_als_plan_host.py (CPU) and
tests/test_gpu_als_forms.py (GPU).

The bound. With u = 2^-24 (float32 unit roundoff), F64 / G64 the float64 contractions of the
float32 inputs and the same contractions of the absolute values

    BF = |W_(n)| (|X| (.) |Y|),     BG = (|X|^T |X|) o (|Y|^T |Y|),

any float32 evaluation satisfies, per element,

    |F - F64| <= (n_F + 4) u BF,    n_F = I J K / dims[n]   (2-way: the reduction length)
    |G - G64| <= (K1 + Kx + 6) u BG (2-way: (K1 + 3) u BG), K1, Kx the factors' row counts.

Derivation (first order in u, every rounding relative to a partial sum of absolute values,
which BF / BG dominate; padded entries are exact zeros and add nothing).
F: every one of the n_F scalar products w x y behind an element is rounded at most once when
the Khatri-Rao value x y is formed and then passes through the roundings of a sum of n_F terms:
in ANY order and grouping that is at most n_F (n_F - 1 additions and the product's own, fewer
with FMAs). The generic form is exactly that (one Khatri-Rao rounding plus a K-term dot
product, K = n_F); a split-K run sums chunk partials in chunk order (a regrouping of the same
n_F - 1 additions). The spatial form regroups the triple sum: modes 0, 1 a J- (I-)term dot
product per tap, one product with the tap factor and a 9-term sum (J + 9 <= 9 J roundings on a
term's path); mode 2 a J-term dot product, one product with the row factor, then the rows of a
tile, the two half-waves, the two waves and the row tiles in order (at most J + I + 1 <= I J
for J >= 2, and the form needs J >= 16). So at most n_F + 1 roundings touch a term:
(n_F + 1) u, one unit for the second-order terms ((n_F + 1)^2 u^2 / 2 < u up to n_F = 5792;
beyond, see TOP below) and two spare: c_F = n_F + 4.
G: each Gram is a K-term dot product (K1, Kx roundings), their product rounds once:
(K1 + Kx + 1) u, second order (K1 + 1)(Kx + 1) u^2 far below u, rounded up to
c_G = K1 + Kx + 6; 2-way: K1 roundings, c_G = K1 + 3. Nothing in either constant is measured.

TOP. At the top of divmod's range (n_F near 2^24) n_F u is about 1 and "any order" would
need the exact (1 + u)^(n_F + 1) - 1 = e - 1. The constant stays n_F + 4 there: the planner
cuts such a reduction into chunks (kchunk 8192, 2048 of them), so a term passes through at most
1 + kchunk + nsplit = 10241 roundings, whose exact worst case (1 + u)^10241 - 1 < 6.2e-4 is
far inside (n_F + 4) u ~ 1. The test asserts the chunking through the plan query. A bound
that large sees little (F itself is about sqrt(n_F), BF about n_F / 2), so the test adds inputs
with entries in {-1, 0, 1}: BF < 2^24 then bounds every partial sum, float32 is exact and F
must equal F64.

What the whole-matrix 1e-5 relative Frobenius norm cannot see and this bound does: a fault in
an element whose own terms are small beside the matrix (a channel of small weights, one
element of a large F); tests/test_als_bound_host.py shows it.
"""
from __future__ import annotations

import functools

import numpy as np

U32 = 2.0 ** -24
GENERIC, GRAM, ERROR, SPATIAL = 0, 1, 2, 3   # job kinds of admmq_debug_cp_plan


def others(ndim: int, mode: int):
    return [d for d in range(ndim) if d != mode]


def n_terms(dims, mode: int) -> int:
    """Scalar products behind one element of F."""
    n = 1
    for d in others(len(dims), mode):
        n *= int(dims[d])
    return n


def f_constant(dims, mode: int) -> float:
    return float(n_terms(dims, mode) + 4)


def g_constant(dims, mode: int) -> float:
    o = others(len(dims), mode)
    return float(dims[o[0]] + 3) if len(o) == 1 else float(dims[o[0]] + dims[o[1]] + 6)


def _mttkrp64(W, fs, mode):
    """W_(mode) KR(others) in float64 without a Khatri-Rao or (I, J, R) intermediate: the
    longer of the two other modes is contracted first (a tensordot), the shorter one after."""
    if W.ndim == 2:
        return (W if mode == 0 else W.T) @ fs[1 - mode]
    a, b = others(3, mode)
    first, second = (a, b) if W.shape[a] >= W.shape[b] else (b, a)
    T = np.tensordot(W, fs[first], axes=([first], [0]))   # (the two remaining modes in order, R)
    rem = [d for d in range(3) if d != first]
    return np.einsum("msr,sr->mr" if rem[0] == mode else "smr,sr->mr", T, fs[second])


def reference(W, factors, mode: int):
    """(G64, F64, BG, BF) in float64 from the float32 inputs (see the module docstring)."""
    W = np.asarray(W, np.float32).astype(np.float64)
    fs = [np.asarray(f, np.float32).astype(np.float64) for f in factors]
    F64 = _mttkrp64(W, fs, mode)
    G64 = np.ones((fs[0].shape[1],) * 2)
    for d in others(W.ndim, mode):
        G64 = G64 * (fs[d].T @ fs[d])
    np.abs(W, out=W)
    fs = [np.abs(f) for f in fs]
    BF = _mttkrp64(W, fs, mode)
    BG = np.ones_like(G64)
    for d in others(W.ndim, mode):
        BG = BG * (fs[d].T @ fs[d])
    return G64, F64, BG, BF


def worst_ratio(got, want, B) -> float:
    """max over the elements of |got - want| / (u B); inf on a non-finite output and where
    B = 0 and the error is not."""
    got = np.asarray(got)
    if got.shape != want.shape or not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(B > 0, err / (U32 * B), np.where(err > 0, np.inf, 0.0))
    return float(q.max())


def rel_frobenius(a, b) -> float:
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@functools.lru_cache(maxsize=None)
def case_inputs(dims, R: int):
    """(W, factors) float32 standard normal, fixed by the shape. Shared: read only."""
    g = np.random.default_rng(7000 * len(dims) + 13 * sum(dims) + R)
    fs = [g.standard_normal((n, R), dtype=np.float32) for n in dims]
    W = g.standard_normal(dims, dtype=np.float32)
    return W, fs


@functools.lru_cache(maxsize=None)
def case_reference(dims, R: int, mode: int):
    W, fs = case_inputs(dims, R)
    return reference(W, fs, mode)


# --------------------------------------------------------------------------------------
# The case table: the smallest shapes that reach each form of plan_als. Per mode the form
# the case is there for, {job kind, BM, nsplit, kchunk} as admmq_debug_cp_plan reports it
# (kchunk 0: the spatial form does not chunk K; its nsplit counts mode 2's row tiles).
# `band`: NaN guard floats on both sides of every operand (64: 16-byte aligned, 65: not).
def _g(BM, nsplit, kchunk):
    return dict(job=GENERIC, BM=BM, nsplit=nsplit, kchunk=kchunk)


def _s(BM, nsplit=1):
    return dict(job=SPATIAL, BM=BM, nsplit=nsplit, kchunk=0)


CASES = [
    # sp<32> in all three modes, 16 of 32 rows masked, one K-step, N = 5
    dict(dims=(16, 16, 9), R=5, band=64, plan=[_s(32), _s(32), _s(32)]),
    # sp<32> modes 0, 2 with full rows, three K-steps, second column tile 6 wide; mode 1 sp<64>, 16 masked rows
    dict(dims=(32, 48, 9), R=70, band=64, plan=[_s(32), _s(64), _s(32)]),
    # sp<32> modes 0, 2 with 12 rows; mode 1 generic BM 32 (I = 12), K = 108, divisor 9
    dict(dims=(12, 32, 9), R=33, band=64, plan=[_s(32), _g(32, 1, 112), _s(32)]),
    # sp<64>, two row tiles (the second 4 rows); mode 2 nsplit 2 through k_als_reduce; mode 1 generic
    dict(dims=(68, 32, 9), R=64, band=64, plan=[_s(64), _g(32, 1, 624), _s(64, 2)]),
    # mode 2 with three row tiles, nsplit 3, N = 9; mode 1 generic split, chunks 608 + 580 (= 36 16 + 4),
    # 608 % 9 != 0: a Khatri-Rao run straddles the chunk boundary
    dict(dims=(132, 16, 9), R=9, band=64, plan=[_s(64), _g(32, 2, 608), _s(64, 3)]),
    # mode 1 sp<64>, three row tiles, last 4 rows, one K-step; modes 0, 2 generic split
    dict(dims=(16, 132, 9), R=40, band=64, plan=[_g(32, 2, 608), _s(64), _g(32, 4, 528)]),
    # one predicate term false at a time
    dict(dims=(16, 24, 9), R=7, band=64, plan=[_g(32, 1, 224), _s(32), _g(32, 1, 384)]),    # J % 16
    dict(dims=(18, 16, 9), R=7, band=64, plan=[_g(32, 1, 144), _g(32, 1, 176), _g(32, 1, 288)]),   # I % 4, I % 16
    dict(dims=(16, 18, 9), R=7, band=64, plan=[_g(32, 1, 176), _g(32, 1, 144), _g(32, 1, 288)]),   # J % 4
    dict(dims=(16, 16, 8), R=7, band=64, plan=[_g(32, 1, 128), _g(32, 1, 128), _g(32, 1, 256)]),   # Kd = 8
    dict(dims=(16, 16, 10), R=7, band=64, plan=[_g(32, 1, 160), _g(32, 1, 160), _g(32, 1, 256)]),  # Kd = 10
    # misaligned W: generic in all modes
    dict(dims=(16, 16, 9), R=5, band=65, plan=[_g(32, 1, 144), _g(32, 1, 144), _g(32, 1, 256)]),
    # 2-way: mode 0 BM 32 split, last chunk 502 = 31 16 + 6; mode 1 1030 rows, K = 5 < 16
    dict(dims=(5, 1030), R=3, band=64, plan=[_g(32, 2, 528), _g(64, 1, 16)]),
    # mode 2 generic afast, K = 1320, divisor 33 (down-correction), chunks 672 + 648 (= 40 16 + 8)
    dict(dims=(40, 33, 5), R=6, band=64, plan=[_g(64, 1, 176), _g(64, 1, 208), _g(32, 2, 672)]),
    # mode 0 generic, K = 1050, divisor 7, split (528 + 522), R = 64 + 1
    dict(dims=(7, 150, 7), R=65, band=64, plan=[_g(32, 2, 528), _g(64, 1, 64), _g(32, 2, 528)]),
    # degenerate extents; Kd = 3 as divisor; Gram with K = 1
    dict(dims=(1, 1, 1), R=1, band=64, plan=[_g(32, 1, 16)] * 3),
    dict(dims=(1, 17, 3), R=40, band=64, plan=[_g(32, 1, 64), _g(32, 1, 16), _g(32, 1, 32)]),
    dict(dims=(1, 1), R=1, band=64, plan=[_g(32, 1, 16)] * 2),
    # Kd = 64: generic 3-way at R past two column tiles
    dict(dims=(9, 64, 64), R=134, band=64, plan=[_g(32, 8, 512), _g(64, 1, 576), _g(64, 1, 576)]),
    # 2-way with both modes on BM 64 and a BM 64 Gram without the Hadamard factor (the plan query
    # showed the table above reaching neither)
    dict(dims=(70, 37), R=40, band=64, plan=[_g(64, 1, 48), _g(64, 1, 80)]),
]


def case_id(c) -> str:
    return "x".join(map(str, c["dims"])) + f"-R{c['R']}" + ("-misaligned" if c["band"] % 4 else "")


def banded(torch, dev, a, band: int):
    """`a` (numpy float32) on the device as the middle of a flat buffer with `band` NaNs on both
    sides (band 64: 16-byte aligned; band 65: 4-byte aligned only). Returns (view, buffer)."""
    buf = torch.full((a.size + 2 * band,), float("nan"), dtype=torch.float32, device=dev)
    v = buf[band:band + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * band) % 16
    return v, buf


def fake_address(band: int) -> int:
    """A W address with the alignment of a `band`-float guard in front (host-only planning)."""
    return 0x100000 + 4 * band


# The mixed batch: both BM classes, both MTTKRP kernels, split and unsplit.
MIXED = [((16, 16, 9), 5), ((68, 32, 9), 64), ((5, 1030), 3), ((40, 33, 5), 6), ((32, 48, 9), 70), ((7, 150, 7), 65)]

# Top of divmod's range: (dims, R, {mode: (nsplit, kchunk) of the generic BM 32 form}).
TOP = [
    # mode 0: K = 16 777 209 < 2^24, divisor 3 (down-correction on a third of the range); mode 2: divisor J
    ((1, 5592403, 3), 2, {0: (2048, 8192), 2: (2045, 2736)}),
    # mode 2: K = 16 777 207, divisor 4099
    ((4093, 4099, 2), 3, {2: (2048, 8192)}),
]
