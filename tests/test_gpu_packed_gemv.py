"""Skinny packed GEMV on the MI355X: k_packed_gemv / k_packed_gemv_t decode exactly
dequantize_packed's weight (one-hot activations: bit-exact), the float32 result meets the derived forward
bound against float64 in the one-launch and the K-split plans, an output's bits depend on its own row of x
only, nothing outside the stream / the output / the workspace is touched, and skinny=True routes by rows."""
import ctypes

import pytest
import torch

from conftest import gpu_available
from test_gpu_packed_hgemm import AFF, DEV, DT, MINMAX, MSE, SCHEMES, SYM, ULP, _hx, _packed, _randn

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SMALL = [(64, 134), (134, 9), (33, 65), (1, 7)]
# (packed shape, transpose): the smallest K-split shapes (K past 1024 for D, 128 for D^T), two chunks a range, and
# rows of whole 16-byte groups for every dtype (K a multiple of 8: x is staged 16 bytes a thread; also K-split)
SPLIT_N, SPLIT_T = ((3, 1025), False), ((129, 5), True)
CHUNKS_N, CHUNKS_T = ((3, 16500), False), ((8300, 5), True)
WIDE_N, WIDE_T = ((3, 1032), False), ((136, 5), True)
SPLITS = [SPLIT_N, SPLIT_T, CHUNKS_N, CHUNKS_T, WIDE_N, WIDE_T]


def _x(shape, seed, dtype):
    return _randn(shape, seed) if dtype == torch.float32 else _hx(shape, seed, dtype)


def _dims(p, trans):
    from admmq.packed import _weight_dims
    return _weight_dims(p, trans)


def _gemv(p, trans, x, bias=None, out_dtype=None):
    from admmq.packed import _meta_words, packed_gemv
    M, K = _dims(p, trans)
    return packed_gemv(p.codes, _meta_words(p), trans, M, K, x, bias, out_dtype)


def _meta(p):
    from admmq import _lib
    from admmq.packed import _meta_words
    return _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())


def _need(p, trans, N):
    from admmq import _lib
    M, K = _dims(p, trans)
    return _lib.load().admmq_packed_gemv_workspace_size(ctypes.byref(_meta(p)), 1 if trans else 0, M, K, N)


@pytest.mark.parametrize("bits,scheme", [(b, s) for b in range(1, 9) for s in SCHEMES if not (s == MINMAX and b == 1)])
def test_one_hot_rows_give_the_decoded_weight(bits, scheme):
    """x = rows of I_K, 8 at a time (the last chunk shorter): the sum is one exact product plus exact zeros and
    the epilogue is dequant_code's operations (tensor_minmax: S_x = 1), so the float32 result is torch.equal to
    dequantize_packed's columns and the half result to their conversion."""
    for shape in SMALL:
        p, D = _packed(shape, bits, scheme)
        for trans in (False, True):
            W = D.T if trans else D                      # [M, K]
            K = W.shape[1]
            for dtype in DTYPES:
                eye = torch.eye(K, device=DEV, dtype=dtype)
                for r0 in range(0, K, 8):
                    what, want = (shape, trans, dtype, r0), W.T[r0:r0 + 8]
                    assert torch.equal(_gemv(p, trans, eye[r0:r0 + 8], None, torch.float32), want), what
                    y = _gemv(p, trans, eye[r0:r0 + 8])
                    assert y.dtype == dtype and torch.equal(y, want.to(dtype)), what


RATIOS = []


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,trans", [(s, t) for s in SMALL for t in (False, True)] + SPLITS)
def test_bound_against_float64(shape, trans, dtype):
    """|y32 - y64| <= (K + 4) 2^-23 mag elementwise, mag = |D||x| + |bias| (tensor_minmax: (|D - mn| + |mn|)|x| +
    |bias|). Derived, not tuned: K FMA roundings, three epilogue roundings, the bias add. Largest ratio measured
    on the MI355X over all cases: see DESIGN.md 2.32."""
    split = (shape, trans) in SPLITS
    for bits, scheme in [(3, AFF), (4, MSE), (8, MINMAX), (4, SYM)]:
        p, D = _packed(shape, bits, scheme)
        assert _need(p, trans, 8) > 0 or not split, (shape, trans)   # the named cases do run the K-split plan
        W64 = (D.T if trans else D).double().cpu()
        M, K = W64.shape
        bias = _randn((M,), 12)
        for N in (1, 3, 8):
            x = _x((N, K), 11 + N, dtype)
            y = _gemv(p, trans, x, bias, torch.float32)
            X64 = x.double().cpu()
            yd = X64 @ W64.T + bias.double().cpu()
            mag = X64.abs() @ ((W64 - p.mn).abs() + abs(p.mn) if scheme == MINMAX else W64.abs()).T + bias.double().cpu().abs()
            err, bound = (y.double().cpu() - yd).abs(), (K + 4) * ULP * mag
            RATIOS.append(float((err / bound.clamp_min(1e-300)).max()))
            print(f"{shape} trans {trans} {dtype} bits {bits} N {N}: max |err| / bound = {RATIOS[-1]:.4f} "
                  f"(largest so far {max(RATIOS):.4f})")
            assert y.dtype == torch.float32 and tuple(y.shape) == (N, M) and bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,trans", [((64, 134), False), ((64, 134), True), ((3, 136), False)] + SPLITS)
def test_an_output_depends_on_its_own_row_only(shape, trans, dtype):
    """Column c of an N = 8 call is the N = 1 call on that row and the matching row of an N = 3 call, a repeated
    call is equal, and the half result is the float32 result converted once - one launch and K split."""
    for scheme in (MSE, MINMAX):
        p, _ = _packed(shape, 4, scheme)
        M, K = _dims(p, trans)
        x, bias = _x((8, K), 17, dtype), _randn((M,), 18)
        y8 = _gemv(p, trans, x, bias, torch.float32)
        assert torch.equal(y8, _gemv(p, trans, x, bias, torch.float32))
        for c in range(8):
            assert torch.equal(_gemv(p, trans, x[c:c + 1], bias, torch.float32)[0], y8[c]), (scheme, c)
        assert torch.equal(_gemv(p, trans, x[5:8], bias, torch.float32), y8[5:8])
        assert torch.equal(_gemv(p, trans, x, bias), y8.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,bits,trans,split", [((33, 65), 3, False, False), ((33, 65), 3, True, False),
                                                    ((5, 1025), 7, False, True), ((129, 5), 7, True, True)])
def test_nothing_outside_the_stream_the_output_or_the_workspace_is_touched(shape, bits, trans, split, dtype):
    """Streams that end one byte after a dword boundary, x one element past a 16-byte boundary; the last two
    cases run the K-split plan and its workspace."""
    from admmq import _lib
    from admmq.packed import packed_bytes
    lib, nbytes, canary = _lib.load(), packed_bytes(shape[0] * shape[1], bits), -12288.0
    assert nbytes % 4 == 1
    for scheme in (SYM, MINMAX):
        p, _ = _packed(shape, bits, scheme)
        M, K = _dims(p, trans)
        need = _need(p, trans, 8)
        assert (need > 0) == split
        x, bias = _x((8, K), 20, dtype), _randn((M,), 21)
        ref = _gemv(p, trans, x, bias)
        xo = torch.empty(x.numel() + 16, device=DEV, dtype=dtype)
        xo = xo[(16 - xo.data_ptr() % 16) % 16 // xo.element_size() + 1:][:x.numel()]
        assert xo.data_ptr() % 16 == xo.element_size()
        xo.copy_(x.reshape(-1))
        outs = []
        for fill in (0x00, 0xFF):
            cbuf = torch.full((64 + nbytes + 512,), fill, dtype=torch.uint8, device=DEV)
            cview = cbuf[64:64 + nbytes]
            assert cview.data_ptr() % 16 == 0
            cview.copy_(p.codes)
            ybuf = torch.full((8 * M + 128,), canary, device=DEV, dtype=dtype)
            ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
            rc = lib.admmq_packed_gemv(_lib.ptr(cview), ctypes.byref(_meta(p)), 1 if trans else 0, M, K, _lib.ptr(xo), DT[dtype],
                                       8, _lib.ptr(bias), _lib.ptr(ybuf[64:]), DT[dtype], _lib.ptr(ws), need,
                                       _lib.stream_handle(DEV))
            assert rc == 0, lib.admmq_last_error()
            torch.cuda.synchronize()
            assert bool((ybuf[:64] == canary).all()) and bool((ybuf[64 + 8 * M:] == canary).all())
            assert bool((ws[need:] == 0xA5).all())
            assert bool((cbuf[:64] == fill).all()) and bool((cbuf[64 + nbytes:] == fill).all())
            outs.append(ybuf[64:64 + 8 * M].clone())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0].view(8, M), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_skinny_routes_by_rows_and_the_two_routes_agree(dtype, monkeypatch):
    from admmq import _lib, export, packed_linear
    for shape, trans in [((70, 134), False), SPLIT_N, SPLIT_T]:
        p, _ = _packed(shape, 4, MSE)
        M, K = _dims(p, trans)
        bias = _randn((M,), 41)
        lin = export.PackedLinear(p, bias, transpose=trans)
        assert lin.skinny is False and "skinny" not in repr(lin) and "skinny" not in str(lin.state_dict().keys())
        x8, x9, x1 = _x((2, 4, K), 42, dtype), _x((9, K), 43, dtype), _x((1, K), 44, dtype)
        today8, today9, today1 = packed_linear(x8, p, bias, trans), packed_linear(x9, p, bias, trans), packed_linear(x1, p, bias, trans)
        assert torch.equal(lin(x8), today8) and torch.equal(packed_linear(x1, p, bias, trans, skinny=False), today1)
        lin.skinny = True
        assert "skinny=True" in repr(lin)
        g8 = _gemv(p, trans, x8.reshape(8, K), bias).reshape(2, 4, M)
        assert torch.equal(packed_linear(x8, p, bias, trans, skinny=True), g8) and torch.equal(lin(x8), g8)
        assert torch.equal(packed_linear(x9, p, bias, trans, skinny=True), today9) and torch.equal(lin(x9), today9)
        assert _lib.use_ops()
        ops = [_gemv(p, trans, x8, bias, od) for od in (None, torch.float32)]
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "use_ops", lambda: False)
            for od, a in zip((None, torch.float32), ops):
                assert torch.equal(_gemv(p, trans, x8, bias, od), a)
                assert torch.equal(packed_linear(x8, p, bias, trans, out_dtype=od, skinny=True), a)
            with pytest.raises(ValueError, match="1..8 rows"):
                _gemv(p, trans, x9, bias)
        with pytest.raises(ValueError, match="1..8 rows"):
            _gemv(p, trans, x9, bias)
        with pytest.raises(RuntimeError, match="inference only"):
            packed_linear(x1.clone().requires_grad_(), p, bias, trans, skinny=True)
