"""Integer quant + low-rank GEMM on the MI355X: k_ilr_down + k_packed_ilrgemm (+ k_packed_ilrreduce)
against a float64 numpy restatement of the contract in include/admmq.h - exact where every intermediate is
representable, packed_linear_int's bits with L = 0, the derived bound on random data, rows alone, guards, the clamp
counter, both binding routes, the builder and the factor sums' stated order."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import gpu_available
from test_gpu_packed_hgemm import AFF, DEV, DTYPES, MSE, SYM, UNIT, _packed, _randn

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

# (M, K, N, r) -> (np, parallel, nsd, launches) of admmq_packed_ilrgemm_plan: what each shape is here for
PLANS = {(134, 134, 70, 24): (3, 1, 3, 3),    # parallel regime, partial last row and column tiles, nsd > 1, r % 32 != 0
         (64, 134, 37, 70): (3, 1, 3, 3),     # three tail steps, two row tiles of the down-projection
         (33, 65, 9, 5): (2, 1, 2, 3),        # a piece (and a range of U) of one k, r % 8 != 0
         (1, 7, 1, 3): (1, 0, 1, 2),          # np = 1, a single partial step
         (1024, 65, 1024, 9): (2, 0, 2, 2)}   # 256 tiles: the serial regime
BITS_SCHEMES = [(3, AFF), (4, MSE), (8, SYM)]
XQ_EXACT = (2, -0.5, 0.75)                    # g = 0.25
OUT_ACT = (4, -2.0, 2.0)


def _codes(shape, bits, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1 << bits, shape, generator=g, dtype=torch.uint8).to(DEV)


def _xq(ux, q):
    from admmq import QuantizedActivation
    return QuantizedActivation(ux, q[0], float(np.float32(q[1])), float(np.float32(q[2])))


def _run(p, L, Rt, xq, bias=None, act=None, out_codes=False, T=torch.bfloat16):
    from admmq import PackedLowRank, packed_lowrank_linear_int
    return packed_lowrank_linear_int(xq, PackedLowRank(q=p, L=L, Rt=Rt), bias, act, out_codes, T)


def _ref(p, D, L, Rt, xq, bias, T, round_t=True):
    """The contract in float64 numpy on the factors as rounded to T: (y64, t64); round_t False: t stays float64."""
    a = np.rint(D.double().cpu().numpy() / np.float64(np.float32(p.scale)))
    ux = xq.codes.cpu().numpy().astype(np.float64)
    gd, mn = np.float64(np.float32(xq.rng)) / ((1 << xq.bits) - 1), np.float64(np.float32(xq.mn))
    LT, RT = L.to(T).double().cpu().numpy(), Rt.to(T).double().cpu().numpy()
    t = gd * (ux @ RT.T) + mn * RT.sum(1)
    tT = torch.from_numpy(t.astype(np.float32)).to(T).double().numpy() if round_t else t
    y = np.float64(np.float32(p.scale)) * (gd * (ux @ a.T) + mn * a.sum(1)) + tT @ LT.T
    return (y if bias is None else y + bias.double().cpu().numpy()), t


def test_the_shapes_run_the_plans_they_are_named_for():
    from admmq import _lib
    for (M, K, N, r), want in PLANS.items():
        out = (ctypes.c_int32 * 4)()
        assert _lib.load().admmq_packed_ilrgemm_plan(M, K, N, r, out) == 0 and tuple(out) == want, (M, K, N, r)


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("shape", list(PLANS))
def test_exact_where_every_intermediate_is_representable(shape, T):
    """L, Rt in {-1, 0, 1} (Rt half zeros), 2-bit codes with g = 0.25, mn_x = -0.5, integer biases: U, t (a multiple
    of 0.25 of at most 8 bits) and q are exact, so y is the float64 formula rounded once. No tolerance."""
    M, K, N, r = shape
    g = torch.Generator().manual_seed(3)
    L = torch.randint(-1, 2, (M, r), generator=g).float().to(DEV)
    Rt = (torch.randint(-1, 2, (r, K), generator=g) * torch.randint(0, 2, (r, K), generator=g)).float().to(DEV)
    bias = torch.randint(-9, 10, (M,), generator=g).float().to(DEV)
    xq = _xq(_codes((N, K), 2, 4), XQ_EXACT)
    for bits, scheme in BITS_SCHEMES:
        p, D = _packed((M, K), bits, scheme)
        want, t = _ref(p, D, L, Rt, xq, bias, T)
        assert (torch.from_numpy(t).to(T).double().numpy() == t).all()   # a condition on the inputs
        want = torch.from_numpy(want.astype(np.float32)).to(DEV)
        for fl, fr in [(L, Rt), (L.to(T), Rt.to(T))]:
            assert torch.equal(_run(p, fl, fr, xq, bias, T=T), want), (bits, scheme, fl.dtype)


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("shape", [(134, 134, 70, 24), (1024, 65, 1024, 9)])
def test_a_zero_L_gives_packed_linear_int(shape, T):
    """q is an exact +0: all three output forms, both regimes, with a bias and without (torch.equal: -0 == +0)."""
    from admmq import packed_linear_int
    M, K, N, r = shape
    L, Rt, bias = torch.zeros(M, r, device=DEV), _randn((r, K), 17, 0.5), _randn((M,), 16)
    xq = _xq(_codes((N, K), 8, 5), (8, -1.3, 1.6))
    for bits, scheme in BITS_SCHEMES:
        p = _packed((M, K), bits, scheme)[0]
        for b in (bias, None):
            assert torch.equal(_run(p, L, Rt, xq, b, T=T), packed_linear_int(xq, p, b))
            assert torch.equal(_run(p, L, Rt, xq, b, OUT_ACT, T=T), packed_linear_int(xq, p, b, act=OUT_ACT))
            got, want = _run(p, L, Rt, xq, b, OUT_ACT, True, T), packed_linear_int(xq, p, b, act=OUT_ACT, out_codes=True)
            assert torch.equal(got.codes, want.codes) and int(got.clamped) == int(want.clamped), (bits, scheme)


RATIOS = []


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("xq3", [(2, -0.5, 0.75), (8, -1.3, 2.9)])
@pytest.mark.parametrize("shape", list(PLANS))
def test_bound_against_float64(shape, xq3, T):
    """|y - y64| <= gamma B + u (1 + gamma) B + eps |y64| elementwise, gamma = (1 + eps)^(K + r + 4) - 1, eps = 2^-23,
    B = |L_T| (|Rt_T| (g ux + |mn_x|)), y64 on the factors as rounded to T with t unrounded.
    Derived, not tuned. Float32 factors and the same factors in T give the same bits. Largest ratio measured on the
    MI355X over all cases: 0.074."""
    M, K, N, r = shape
    eps, u = 2.0 ** -23, UNIT[T]
    gam = (1.0 + eps) ** (K + r + 4) - 1.0
    L, Rt, bias = _randn((M, r), 5 + M + r, 0.5).to(T), _randn((r, K), 6 + K + r, 0.5).to(T), _randn((M,), 12)
    xq = _xq(_codes((N, K), xq3[0], 11 + N), xq3)
    xabs = xq.codes.cpu().numpy().astype(np.float64) * (np.float64(np.float32(xq.rng)) / ((1 << xq.bits) - 1)) + abs(xq.mn)
    B = (xabs @ np.abs(Rt.double().cpu().numpy()).T) @ np.abs(L.double().cpu().numpy()).T
    for bits, scheme in BITS_SCHEMES:
        p, D = _packed((M, K), bits, scheme)
        y = _run(p, L.float(), Rt.float(), xq, bias, T=T)
        assert torch.equal(y, _run(p, L, Rt, xq, bias, T=T)), (bits, scheme)
        y64 = _ref(p, D, L, Rt, xq, bias, T, round_t=False)[0]
        err, bound = np.abs(y.double().cpu().numpy() - y64), gam * B + u * (1 + gam) * B + eps * np.abs(y64)
        RATIOS.append(float((err / np.maximum(bound, 1e-300)).max()))
        print(f"{shape} {T} x bits {xq3[0]} w bits {bits} {scheme}: max |err| / bound = {RATIOS[-1]:.4f} (largest so far {max(RATIOS):.4f})")
        assert tuple(y.shape) == (N, M) and bool((err <= bound).all())


@pytest.mark.parametrize("T", DTYPES)
def test_rows_alone_repeats_canaries_and_an_odd_address(T):
    """Rows of a 70-row call against the same rows alone (one regime, one plan of U) and a repeated call; then
    canaries round y / y_codes and behind the stated workspace bytes with ux one byte past a 16-byte boundary and
    factors in T of r % 8 != 0, through ctypes."""
    from admmq import _lib, packed_lowrank_factorsums, packed_rowsums, PackedLowRank
    from admmq.packed import HALF_DTYPES, _meta_words
    M, K, N, r = 134, 134, 70, 5
    p = _packed((M, K), 4, MSE)[0]
    L, Rt, bias = _randn((M, r), 21, 0.5), _randn((r, K), 22, 0.5), _randn((M,), 23)
    xq = _xq(_codes((N, K), 8, 24), (8, -1.3, 2.9))
    y = _run(p, L, Rt, xq, bias, T=T)
    assert torch.equal(y, _run(p, L, Rt, xq, bias, T=T))
    for c in (0, 36, 69):
        assert torch.equal(_run(p, L, Rt, _xq(xq.codes[c:c + 1].clone(), (8, -1.3, 2.9)), bias, T=T)[0], y[c]), c
    lib, LT, RT = _lib.load(), L.to(T).contiguous(), Rt.to(T).contiguous()
    rho, rs = packed_lowrank_factorsums(PackedLowRank(q=p, L=LT, Rt=RT), T), packed_rowsums(p)
    need = lib.admmq_packed_ilrgemm_workspace_size(M, K, N, r)
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    xbuf = torch.zeros(N * K + 32, dtype=torch.uint8, device=DEV)
    xbuf[17:17 + N * K] = xq.codes.reshape(-1)
    xr, oq = _lib.ActQ(8, 1, xq.mn, xq.rng), _lib.ActQ(4, 1, -2.0, 4.0)
    for out_codes in (False, True):
        ybuf = torch.full((N * M + 64,), 7 if out_codes else -77.0, dtype=torch.uint8 if out_codes else torch.float32, device=DEV)
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        cl = torch.full((3,), -5, dtype=torch.int32, device=DEV)
        yp = ybuf[32:32 + N * M]
        rc = lib.admmq_packed_ilrgemm(_lib.ptr(p.codes), ctypes.byref(meta), M, K, _lib.ptr(LT), _lib.ptr(RT), HALF_DTYPES[T],
                                      HALF_DTYPES[T], r, _lib.ptr(rho), _lib.ptr(xbuf[17:]), ctypes.byref(xr), _lib.ptr(rs), N,
                                      _lib.ptr(bias), None if out_codes else _lib.ptr(yp), _lib.ptr(yp) if out_codes else None,
                                      ctypes.byref(oq) if out_codes else None, _lib.ptr(cl[1:]) if out_codes else None,
                                      _lib.ptr(ws), need, _lib.stream_handle(DEV))
        assert rc == 0, lib.admmq_last_error()
        want = _run(p, L, Rt, xq, bias, (4, -2.0, 2.0), True, T) if out_codes else y
        assert torch.equal(yp.view(N, M), want.codes if out_codes else want)
        pad = 7 if out_codes else -77.0
        assert bool((ybuf[:32] == pad).all()) and bool((ybuf[32 + N * M:] == pad).all()) and bool((ws[need:] == 0xA5).all())
        if out_codes:
            assert cl.tolist() == [-5, int(want.clamped), -5]


@pytest.mark.parametrize("shape", [(134, 134, 70, 24), (1024, 65, 1024, 9)])
def test_the_clamp_counter_counts_the_reference_encode(shape):
    """A 3-bit output range that the outputs overrun: codes and count equal the float32 encode of the float output."""
    M, K, N, r = shape
    p = _packed((M, K), 4, MSE)[0]
    L, Rt, bias = _randn((M, r), 31, 0.5), _randn((r, K), 32, 0.5), _randn((M,), 33)
    xq = _xq(_codes((N, K), 8, 34), (8, -1.3, 2.9))
    y, got = _run(p, L, Rt, xq, bias), _run(p, L, Rt, xq, bias, (3, -1.0, 1.0), True)
    qi = torch.floor(((y - got.mn) / np.float32(got.rng)) * 7.0 + 0.5)
    assert int(got.clamped) == int(((qi < 0) | (qi > 7) | qi.isnan()).sum()) > 0
    assert torch.equal(got.codes, qi.clamp(0, 7).to(torch.uint8))


def test_bindings_builder_and_state(monkeypatch):
    """ops route == ctypes route; build_qlr_layer(integer=True) == act_encode + the call; its state dict round-trips;
    without integer the builder returns today's module."""
    import admmq
    from admmq import _lib, export
    M, K, N, r = 33, 65, 9, 5
    p = _packed((M, K), 4, SYM)[0]
    pl = admmq.PackedLowRank(q=p, L=_randn((M, r), 41, 0.5), Rt=_randn((r, K), 42, 0.5))
    bias, x = _randn((M,), 43), _randn((2, N, K), 44, 0.4)
    act = (8, -2.0, 2.0)
    xq = admmq.act_encode(x, act, check=False)
    y = admmq.packed_lowrank_linear_int(xq, pl, bias, tail_dtype=torch.float16)
    assert tuple(y.shape) == (2, N, M) and y.dtype == torch.float32
    monkeypatch.setattr(_lib, "use_ops", lambda: False)
    pl2 = admmq.PackedLowRank(q=p, L=pl.L, Rt=pl.Rt)   # (a fresh cache: the factor sums through ctypes too)
    assert torch.equal(admmq.packed_lowrank_linear_int(xq, pl2, bias, tail_dtype=torch.float16), y)
    monkeypatch.undo()
    lay = export.build_qlr_layer(pl, bias, integer=True, in_act=act, tail_dtype=torch.float16)
    assert isinstance(lay, export.IntegerPackedLowRank) and torch.equal(lay(x), y)
    assert type(export.build_qlr_layer(pl, bias)) is export.PackedLowRankLinear
    other = admmq.PackedLowRank(q=_packed((M, K), 4, SYM, 9)[0], L=torch.zeros_like(pl.L), Rt=torch.zeros_like(pl.Rt))
    lay2 = export.build_qlr_layer(other, torch.zeros_like(bias), integer=True, in_act=(4, -1.0, 1.0))
    lay2.load_state_dict(lay.state_dict())
    assert lay2.tail_dtype == torch.float16 and torch.equal(lay2(x), y)


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("r,K", [(5, 135), (3, 7), (70, 64)])
def test_factor_sums_in_the_stated_order(r, K, T):
    """One wave a row: lane l adds k = l, l + 64, ... in double in increasing k, the 64 partials in increasing l."""
    from admmq.packed import _factorsums
    Rt = _randn((r, K), 51 + K, 0.5)
    RT = Rt.to(T).double().cpu().numpy()
    want = np.zeros(r)
    for j in range(r):
        part = np.zeros(64)
        for k in range(K):
            part[k % 64] += RT[j, k]
        s = part[0]
        for l in range(1, 64):
            s = s + part[l]
        want[j] = s
    for f in (Rt, Rt.to(T)):
        assert np.array_equal(_factorsums(f, T).cpu().numpy(), want.astype(np.float32))
