"""Half-precision fused quant + low-rank GEMM on the MI355X: k_hlr_down + k_packed_hlrgemm
(+ k_packed_hlrreduce) give exactly (v + q) + bias on data where q is exact, packed_linear's bits with L = 0, meet
the derived bound against float64 with float32 and half factors bit-equal, a row's bits depend on that row only,
nothing outside the output / the workspace is touched, and fused=True routes behind skinny."""
import ctypes

import pytest
import torch

from conftest import gpu_available
from test_gpu_packed_hgemm import AFF, DEV, DT, DTYPES, MINMAX, MSE, SYM, ULP, UNIT, _hx, _packed, _randn

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

# (M, K, N, r) -> (np, parallel, nsd, launches) of admmq_packed_hlrgemm_plan: what each shape is here for
PLANS = {(64, 134, 37, 1): (3, 1, 3, 3), (64, 134, 37, 31): (3, 1, 3, 3), (64, 134, 37, 33): (3, 1, 3, 3),
         (64, 134, 37, 256): (3, 1, 3, 3),    # parallel regime, a split down-projection, tail steps 1 and 8, r % 8 != 0
         (134, 134, 70, 24): (3, 1, 3, 3),    # partial last row tile and partial last column tile
         (33, 65, 9, 5): (2, 1, 2, 3),        # a piece (and a range of t) of one k
         (1, 7, 1, 3): (1, 0, 1, 2),          # np = 1, a single partial step
         (1024, 65, 1024, 9): (2, 0, 2, 2)}   # 256 tiles: the serial regime with np = 2
BITS_SCHEMES = [(3, AFF), (4, MSE), (8, MINMAX), (4, SYM)]
ETA = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}   # half a subnormal spacing: t's rounding below the normal range


def _meta(p):
    from admmq import _lib
    from admmq.packed import _meta_words
    return _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())


def _hlr(p, L, Rt, x, bias=None, out_dtype=None):
    from admmq.packed import _meta_words, packed_hlrgemm
    return packed_hlrgemm(p.codes, _meta_words(p), p.shape[0], p.shape[1], L, Rt, x, bias, out_dtype)


def _signs(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-1, 2, shape, generator=g).to(dtype)).to(DEV)


def test_the_shapes_run_the_plans_they_are_named_for():
    from admmq import _lib
    for (M, K, N, r), want in PLANS.items():
        out = (ctypes.c_int32 * 4)()
        assert _lib.load().admmq_packed_hlrgemm_plan(ctypes.byref(_meta(_packed((M, K), 4, MSE)[0])), M, K, N, r, out) == 0
        assert tuple(out) == want, (M, K, N, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(PLANS))
def test_exact_on_sign_data(shape, dtype):
    """x, Rt, L in {-1, 0, 1}: |t| <= K <= 256 is exact in both half types and q is exact in float32, so
    y32 == (v + q) + bias with v the existing half kernel's float32 result, q from float64 on the CPU and the two
    adds made in float32 by torch; the half output is that converted once. No tolerance."""
    from admmq import packed_linear
    M, K, N, r = shape
    x, bias = _signs((N, K), 3, dtype), _randn((M,), 4)
    L, Rt = _signs((M, r), 5), _signs((r, K), 6)
    q = ((x.double().cpu() @ Rt.double().cpu().T) @ L.double().cpu().T).float().to(DEV)
    for bits, scheme in BITS_SCHEMES:
        p = _packed((M, K), bits, scheme)[0]
        want = (packed_linear(x, p, out_dtype=torch.float32) + q) + bias
        for fl, fr in [(L, Rt), (L.to(dtype), Rt.to(dtype))]:
            y32 = _hlr(p, fl, fr, x, bias, torch.float32)
            assert y32.dtype == torch.float32 and torch.equal(y32, want), (bits, scheme, fl.dtype)
            y = _hlr(p, fl, fr, x, bias)
            assert y.dtype == dtype and torch.equal(y, want.to(dtype)), (bits, scheme, fl.dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(64, 134, 37, 33), (1024, 65, 1024, 9)])
def test_a_zero_L_gives_packed_linear(shape, dtype):
    """q is an exact +0, so (v + 0) + bias is the half route's packed_linear, in both regimes (torch.equal: -0 == +0)."""
    from admmq import packed_linear
    M, K, N, r = shape
    x, bias, Rt = _hx((N, K), 15, dtype), _randn((M,), 16), _randn((r, K), 17, 0.5)
    for scheme in (MSE, MINMAX):
        p = _packed((M, K), 4, scheme)[0]
        for b in (bias, None):
            for od in (None, torch.float32):
                assert torch.equal(_hlr(p, torch.zeros(M, r, device=DEV), Rt, x, b, od), packed_linear(x, p, b, out_dtype=od)), (scheme, od)


RATIOS = []


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(PLANS))
def test_bound_against_float64(shape, dtype):
    """|y32 - y64| <= g (A + B + |bias|) + u (1 + g) B + eta (1 + g) |L| 1 elementwise, g = (1 + 2^-23)^(K + r + 6) - 1,
    A = |D||x| (tensor_minmax: (|D - mn| + |mn|)|x|, its two sums), B = |L|(|Rt||x|), u = 2^-8 / 2^-11 the one rounding
    of t, eta = 2^-25 where a float16 t is subnormal (first order (K + r + 6) 2^-23 (A + B + |bias|) + u B).
    Derived, not tuned. The factors are rounded to x's dtype first and passed once as float32 and once as that dtype:
    the same bits. Largest ratio measured on the MI355X over all cases: 0.262."""
    M, K, N, r = shape
    u, g = UNIT[dtype], (1.0 + ULP) ** (K + r + 6) - 1.0
    L, Rt = _randn((M, r), 5 + M + r, 0.5).to(dtype), _randn((r, K), 6 + K + r, 0.5).to(dtype)
    x, bias = _hx((N, K), 11 + N, dtype), _randn((M,), 12)
    X64, L64, R64, b64 = x.double().cpu(), L.double().cpu(), Rt.double().cpu(), bias.double().cpu()
    B = (X64.abs() @ R64.abs().T) @ L64.abs().T
    for bits, scheme in BITS_SCHEMES:
        p, D = _packed((M, K), bits, scheme)
        D64 = D.double().cpu()
        Dmag = (D64 - p.mn).abs() + abs(p.mn) if scheme == MINMAX else D64.abs()
        y = _hlr(p, L.float(), Rt.float(), x, bias, torch.float32)
        assert torch.equal(y, _hlr(p, L, Rt, x, bias, torch.float32)), (bits, scheme)
        yd = X64 @ (D64 + L64 @ R64).T + b64
        bound = g * (X64.abs() @ Dmag.T + B + b64.abs()) + u * (1 + g) * B + ETA[dtype] * (1 + g) * L64.abs().sum(1)
        err = (y.double().cpu() - yd).abs()
        RATIOS.append(float((err / bound.clamp_min(1e-300)).max()))
        print(f"{shape} {dtype} bits {bits} {scheme}: max |err| / bound = {RATIOS[-1]:.4f} (largest so far {max(RATIOS):.4f})")
        assert tuple(y.shape) == (N, M) and bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_depends_on_itself_only_and_nothing_else_is_touched(dtype):
    """Rows of a 37-row call against the same rows alone and a repeated call (one regime, one plan of t); then
    canaries round y and behind the stated workspace bytes with x one element past a 16-byte boundary and half
    factors of r % 8 != 0 (rows of L off 16-byte boundaries), through ctypes."""
    from admmq import _lib
    lib, canary = _lib.load(), -12288.0
    M, K, N, r = 64, 134, 37, 33
    L, Rt = _randn((M, r), 21, 0.5).to(dtype), _randn((r, K), 22, 0.5).to(dtype)
    x, bias = _hx((N, K), 23, dtype), _randn((M,), 24)
    for scheme in (SYM, MINMAX):
        p = _packed((M, K), 7, scheme)[0]
        ref = _hlr(p, L, Rt, x, bias)
        assert torch.equal(ref, _hlr(p, L, Rt, x, bias))
        assert torch.equal(_hlr(p, L, Rt, x[5:6], bias), ref[5:6]) and torch.equal(_hlr(p, L, Rt, x[30:], bias), ref[30:])
        need = lib.admmq_packed_hlrgemm_workspace_size(ctypes.byref(_meta(p)), M, K, N, r)
        xo = torch.empty(x.numel() + 16, device=DEV, dtype=dtype)
        xo = xo[(16 - xo.data_ptr() % 16) % 16 // 2 + 1:][:x.numel()]
        assert xo.data_ptr() % 16 == 2 and need > 0
        xo.copy_(x.reshape(-1))
        ybuf = torch.full((N * M + 128,), canary, device=DEV, dtype=dtype)
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        rc = lib.admmq_packed_hlrgemm(_lib.ptr(p.codes), ctypes.byref(_meta(p)), M, K, _lib.ptr(L), _lib.ptr(Rt), DT[dtype], r,
                                      _lib.ptr(xo), DT[dtype], N, _lib.ptr(bias), _lib.ptr(ybuf[64:]), DT[dtype], _lib.ptr(ws), need,
                                      _lib.stream_handle(DEV))
        assert rc == 0, lib.admmq_last_error()
        torch.cuda.synchronize()
        assert bool((ybuf[:64] == canary).all()) and bool((ybuf[64 + N * M:] == canary).all())
        assert bool((ws[need:] == 0xA5).all())
        assert torch.equal(ybuf[64:64 + N * M].view(N, M), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_routing_the_two_bindings_and_a_converted_module(dtype, monkeypatch):
    """skinny first (8 rows), then fused (9 rows, and 8 rows without skinny), else today's call; the ops and ctypes
    routes are equal; a PackedLowRankLinear with representable factors and bias gives the same bits after .to(dtype)."""
    from admmq import PackedLowRank, _lib, export, packed_lowrank_linear, packed_lrgemv
    from admmq.packed import _meta_words
    M, K, r = 70, 134, 33
    q = _packed((M, K), 4, MSE)[0]
    L, Rt, bias = _randn((M, r), 31, 0.5).to(dtype).float(), _randn((r, K), 32, 0.5).to(dtype).float(), _randn((M,), 33).to(dtype).float()
    p = PackedLowRank(q=q, L=L, Rt=Rt)
    x8, x9 = _hx((2, 4, K), 34, dtype), _hx((9, K), 35, dtype)
    f8, f9 = _hlr(q, L, Rt, x8, bias), _hlr(q, L, Rt, x9, bias)
    today9 = packed_lowrank_linear(x9, p, bias)
    assert torch.equal(packed_lowrank_linear(x9, p, bias, fused=False), today9)
    assert torch.equal(packed_lowrank_linear(x9.float(), p, bias, fused=True), packed_lowrank_linear(x9.float(), p, bias))
    assert torch.equal(packed_lowrank_linear(x9, p, bias, skinny=True, fused=True), f9)
    assert torch.equal(packed_lowrank_linear(x8, p, bias, fused=True), f8)
    g8 = packed_lrgemv(q.codes, _meta_words(q), M, K, L, Rt, x8, bias)
    assert torch.equal(packed_lowrank_linear(x8, p, bias, skinny=True, fused=True), g8)
    lin = export.PackedLowRankLinear(p, bias)
    assert torch.equal(lin(x9), today9)
    lin.fused = lin.skinny = True
    assert torch.equal(lin(x9), f9) and torch.equal(lin(x8), g8)
    lin = lin.to(dtype)
    assert lin.L.dtype == dtype and lin.bias.dtype == dtype and torch.equal(lin(x9), f9)
    assert _lib.use_ops()
    o8 = _hlr(q, L.to(dtype), Rt.to(dtype), x8, bias, torch.float32)
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "use_ops", lambda: False)
        assert torch.equal(_hlr(q, L, Rt, x9, bias), f9)
        assert torch.equal(_hlr(q, L.to(dtype), Rt.to(dtype), x8, bias, torch.float32), o8)
    with pytest.raises(TypeError, match="packed_lrgemm"):
        _hlr(q, L, Rt, x9.float(), bias)
    with pytest.raises(RuntimeError, match="inference only"):
        packed_lowrank_linear(x9.clone().requires_grad_(), p, bias, fused=True)
