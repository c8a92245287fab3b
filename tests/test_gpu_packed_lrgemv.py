"""Skinny quant + low-rank GEMV on the MI355X: k_lr_down_gemv + k_packed_lrgemv meet the derived
forward bound against float64 in every plan, give packed_gemv's bits with L = 0, an output's bits depend on its
own row of x only, nothing outside the output / the workspace is touched, and skinny=True routes by rows."""
import ctypes

import pytest
import torch

from conftest import gpu_available
from test_gpu_packed_hgemm import AFF, DEV, DT, MINMAX, MSE, SYM, ULP, _hx, _packed, _randn

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
C_EXTRA = 29           # include/admmq.h: 15 range adds of t + 7 (t's lane tree) + 5 (q's lane tree) + 2 (v + q, + bias)
SPLIT = (3, 1025)      # the smallest K-split of the code sum (ns = 2)
DOWN_SPLIT = (5, 257)  # with r = 1 the smallest (K, r) whose down-projection is split: ranges of 256 k and 1 k
CASES = [((64, 134), r) for r in (1, 31, 33, 256)] + [((33, 65), 5), ((1, 7), 3), (SPLIT, 9), (DOWN_SPLIT, 1)]


def _x(shape, seed, dtype):
    return _randn(shape, seed) if dtype == torch.float32 else _hx(shape, seed, dtype)


def _factors(shape, r):
    (M, K) = shape
    return _randn((M, r), 5 + M + r, 0.5), _randn((r, K), 6 + K + r, 0.5)


def _meta(p):
    from admmq import _lib
    from admmq.packed import _meta_words
    return _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())


def _plan(p, r):
    """(ns, nsd, launches) of admmq_packed_lrgemv_plan."""
    from admmq import _lib
    out = (ctypes.c_int32 * 3)()
    assert _lib.load().admmq_packed_lrgemv_plan(ctypes.byref(_meta(p)), p.shape[0], p.shape[1], r, out) == 0
    return tuple(out)


def _lrgemv(p, L, Rt, x, bias=None, out_dtype=None):
    from admmq.packed import _meta_words, packed_lrgemv
    return packed_lrgemv(p.codes, _meta_words(p), p.shape[0], p.shape[1], L, Rt, x, bias, out_dtype)


def _gemv(p, x, bias=None, out_dtype=None):
    from admmq.packed import _meta_words, packed_gemv
    return packed_gemv(p.codes, _meta_words(p), False, p.shape[0], p.shape[1], x, bias, out_dtype)


def test_the_shapes_run_the_plans_they_are_named_for():
    p = _packed(SPLIT, 4, MSE)[0]
    assert _plan(p, 9) == (2, 5, 3) and _plan(_packed((64, 134), 4, MSE)[0], 33) == (1, 1, 2)
    p = _packed(DOWN_SPLIT, 4, MSE)[0]
    assert _plan(p, 1) == (1, 2, 2)                             # ranges [0, 256) and [256, 257): one k of a chunk
    assert _plan(_packed((5, 256), 4, MSE)[0], 1)[1] == 1       # one k fewer: one range


RATIOS = []


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,r", CASES)
def test_bound_against_float64(shape, r, dtype):
    """|y32 - y64| <= 2^-23 [(K + 4)(|D||x| + |bias|) + (K + r + c)|L|(|Rt||x|)] elementwise, c = 29 the extra
    roundings of the written order (include/admmq.h); tensor_minmax with (|D - mn| + |mn|)|x|. Derived, not
    tuned. A half x also runs with factors of its own dtype (the reference from those values). Largest ratio
    measured on the MI355X over all cases: see DESIGN.md 2.33."""
    M, K = shape
    L, Rt = _factors(shape, r)
    bias = _randn((M,), 12)
    b64 = bias.double().cpu()
    for bits, scheme in [(3, AFF), (4, MSE), (8, MINMAX), (4, SYM)]:
        p, D = _packed(shape, bits, scheme)
        D64 = D.double().cpu()
        Dmag = (D64 - p.mn).abs() + abs(p.mn) if scheme == MINMAX else D64.abs()
        for N in (1, 3, 8):
            x = _x((N, K), 11 + N, dtype)
            X64 = x.double().cpu()
            for fl, fr in [(L, Rt)] + ([(L.to(dtype), Rt.to(dtype))] if dtype != torch.float32 and N == 3 else []):
                y = _lrgemv(p, fl, fr, x, bias, torch.float32)
                L64, R64 = fl.double().cpu(), fr.double().cpu()
                yd = X64 @ (D64 + L64 @ R64).T + b64
                bound = ULP * ((K + 4) * (X64.abs() @ Dmag.T + b64.abs()) +
                               (K + r + C_EXTRA) * ((X64.abs() @ R64.abs().T) @ L64.abs().T))
                err = (y.double().cpu() - yd).abs()
                RATIOS.append(float((err / bound.clamp_min(1e-300)).max()))
                print(f"{shape} r {r} {dtype} factors {fl.dtype} bits {bits} N {N}: max |err| / bound = {RATIOS[-1]:.4f} "
                      f"(largest so far {max(RATIOS):.4f})")
                assert y.dtype == torch.float32 and tuple(y.shape) == (N, M) and bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(64, 134), SPLIT])
def test_a_zero_L_gives_packed_gemv(shape, dtype):
    """q is an exact +0, so (v + 0) + bias is packed_gemv's value, in both plans (torch.equal: -0 == +0)."""
    L, Rt = _factors(shape, 33)
    for scheme in (MSE, MINMAX):
        p, _ = _packed(shape, 4, scheme)
        x, bias = _x((8, shape[1]), 15, dtype), _randn((shape[0],), 16)
        for b in (bias, None):
            for od in (None, torch.float32):
                assert torch.equal(_lrgemv(p, torch.zeros_like(L), Rt, x, b, od), _gemv(p, x, b, od)), (scheme, od)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,r", [((64, 134), 33), (SPLIT, 9), (DOWN_SPLIT, 1)])
def test_an_output_depends_on_its_own_row_only(shape, r, dtype):
    """Column c of an N = 8 call is the N = 1 call on that row and the matching row of an N = 3 call, a repeated
    call is equal, and the half result is the float32 result on x.float() converted once."""
    L, Rt = _factors(shape, r)
    for scheme in (MSE, MINMAX):
        p, _ = _packed(shape, 4, scheme)
        x, bias = _x((8, shape[1]), 17, dtype), _randn((shape[0],), 18)
        y8 = _lrgemv(p, L, Rt, x, bias, torch.float32)
        assert torch.equal(y8, _lrgemv(p, L, Rt, x, bias, torch.float32))
        for c in range(8):
            assert torch.equal(_lrgemv(p, L, Rt, x[c:c + 1], bias, torch.float32)[0], y8[c]), (scheme, c)
        assert torch.equal(_lrgemv(p, L, Rt, x[5:8], bias, torch.float32), y8[5:8])
        assert torch.equal(_lrgemv(p, L, Rt, x.float(), bias), y8)
        assert torch.equal(_lrgemv(p, L, Rt, x, bias), y8.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,r,split", [((33, 65), 5, False), ((5, 1025), 5, True)])
def test_nothing_outside_the_output_or_the_workspace_is_touched(shape, r, split, dtype):
    """Canaries round y and behind the stated workspace bytes, x one element past a 16-byte boundary, L rows off
    16-byte boundaries; one shape per plan."""
    from admmq import _lib
    lib, canary = _lib.load(), -12288.0
    M, K = shape
    L, Rt = _factors(shape, r)
    for scheme in (SYM, MINMAX):
        p, _ = _packed(shape, 7, scheme)
        need = lib.admmq_packed_lrgemv_workspace_size(ctypes.byref(_meta(p)), M, K, 8, r)
        assert (_plan(p, r)[0] > 1) == split and need > 0
        x, bias = _x((8, K), 20, dtype), _randn((M,), 21)
        ref = _lrgemv(p, L, Rt, x, bias)
        xo = torch.empty(x.numel() + 16, device=DEV, dtype=dtype)
        xo = xo[(16 - xo.data_ptr() % 16) % 16 // xo.element_size() + 1:][:x.numel()]
        assert xo.data_ptr() % 16 == xo.element_size()
        xo.copy_(x.reshape(-1))
        ybuf = torch.full((8 * M + 128,), canary, device=DEV, dtype=dtype)
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        rc = lib.admmq_packed_lrgemv(_lib.ptr(p.codes), ctypes.byref(_meta(p)), M, K, _lib.ptr(L), _lib.ptr(Rt), 0, r, _lib.ptr(xo),
                                     DT[dtype], 8, _lib.ptr(bias), _lib.ptr(ybuf[64:]), DT[dtype], _lib.ptr(ws), need,
                                     _lib.stream_handle(DEV))
        assert rc == 0, lib.admmq_last_error()
        torch.cuda.synchronize()
        assert bool((ybuf[:64] == canary).all()) and bool((ybuf[64 + 8 * M:] == canary).all())
        assert bool((ws[need:] == 0xA5).all())
        assert torch.equal(ybuf[64:64 + 8 * M].view(8, M), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_skinny_routes_by_rows_and_the_two_routes_agree(dtype, monkeypatch):
    """8 and 1 rows take the skinny route, 9 rows and skinny=False today's. The routes agree within the sum of
    their bounds: the skinny one's above, and for today's (K + r + 6) 2^-23 mag - the GEMM's K + 4, the r terms
    of the tail and two adds, every float32 operation at one full ulp."""
    from admmq import PackedLowRank, _lib, export, packed_lowrank_linear
    for shape, r in [((70, 134), 33), (SPLIT, 9)]:
        M, K = shape
        q, D = _packed(shape, 4, MSE)
        L, Rt = _factors(shape, r)
        p, bias = PackedLowRank(q=q, L=L, Rt=Rt), _randn((M,), 41)
        lin = export.PackedLowRankLinear(p, bias)
        assert lin.skinny is False and "skinny" not in repr(lin) and "skinny" not in str(lin.state_dict().keys())
        x8, x9, x1 = _x((2, 4, K), 42, dtype), _x((9, K), 43, dtype), _x((1, K), 44, dtype)
        today8, today9 = packed_lowrank_linear(x8, p, bias), packed_lowrank_linear(x9, p, bias)
        assert torch.equal(lin(x8), today8) and torch.equal(packed_lowrank_linear(x8, p, bias, skinny=False), today8)
        lin.skinny = True
        assert "skinny=True" in repr(lin) and "skinny" not in str(lin.state_dict().keys())
        g8 = _lrgemv(q, L, Rt, x8.reshape(8, K), bias).reshape(2, 4, M)
        assert torch.equal(packed_lowrank_linear(x8, p, bias, skinny=True), g8) and torch.equal(lin(x8), g8)
        assert torch.equal(lin(x1), _lrgemv(q, L, Rt, x1, bias))
        assert torch.equal(packed_lowrank_linear(x9, p, bias, skinny=True), today9) and torch.equal(lin(x9), today9)
        X64 = x8.reshape(8, K).double().cpu().abs()
        magD, magL = X64 @ D.double().cpu().abs().T + bias.double().cpu().abs(), (X64 @ Rt.double().cpu().abs().T) @ L.double().cpu().abs().T
        bound = ULP * ((K + 4) * magD + (K + r + C_EXTRA) * magL + (K + r + 6) * (magD + magL))
        a = packed_lowrank_linear(x8, p, bias, torch.float32, skinny=True).reshape(8, M).double().cpu()
        b = packed_lowrank_linear(x8, p, bias, torch.float32).reshape(8, M).double().cpu()
        assert bool(((a - b).abs() <= bound).all())
        assert _lib.use_ops()
        ops = [_lrgemv(q, L, Rt, x8, bias, od) for od in (None, torch.float32)]
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "use_ops", lambda: False)
            for od, want in zip((None, torch.float32), ops):
                assert torch.equal(_lrgemv(q, L, Rt, x8, bias, od), want)
                assert torch.equal(packed_lowrank_linear(x8, p, bias, od, skinny=True), want)
            with pytest.raises(ValueError, match="1..8 rows"):
                _lrgemv(q, L, Rt, x9, bias)
        with pytest.raises(ValueError, match="1..8 rows"):
            _lrgemv(q, L, Rt, x9, bias)
        with pytest.raises(RuntimeError, match="inference only"):
            packed_lowrank_linear(x1.clone().requires_grad_(), p, bias, skinny=True)
