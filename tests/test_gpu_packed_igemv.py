"""Skinny integer GEMV on the MI355X: k_packed_igemv / k_packed_igemv_t equal the numpy
oracle of the integer contract (int64 sums, the double formula, one rounding) and packed_linear_int's default
route bit for bit - every width, scheme, orientation, output form and plan - hold at the sum's limit K = 65536,
write nothing else, and skinny=True routes by rows."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import gpu_available
from test_gpu_packed_igemm import (AFF, DEV, MSE, SYM, XMN, XRNG, _bits_equal, _codes, _factors, _oracle_layout, _randn,
                                   _weight, _xq)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

# packed shapes: W = D [33, 65] is a full and a partial 32-row tile; W = D^T [261, 65] a full and a partial 256-m
# tile. K = 65 is odd, leaves a tail of one k behind a 16-byte group / a wave's 64 k, and no row of either stream
# (65 or 261 codes) ends on a dword boundary at any width.
SMALL = {False: (33, 65), True: (65, 261)}


def _plan(p, trans):
    """(M, K, ks, ns) of admmq_packed_igemv_plan for p in one orientation."""
    from admmq import _lib
    from admmq.packed import _meta_words, _weight_dims
    M, K = _weight_dims(p, trans)
    meta, out = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes()), (ctypes.c_int32 * 3)()
    assert _lib.load().admmq_packed_igemv_plan(ctypes.byref(meta), 1 if trans else 0, M, K, out) == 0
    return M, K, out[0], out[1]


def _split_shape(trans, bits, rows, chunks):
    """The packed shape with `rows` rows of W whose K is the smallest the plan splits (chunks = 1), or an odd K
    past it at bits whose range minimum is two chunks (chunks = 2) - read from the plan query."""
    from test_packed_hgemm_host import _host_packed
    split = lambda k: _plan(_host_packed((k, rows) if trans else (rows, k), bits), trans)[2:]   # noqa: E731
    lo, hi = 1, 65536                       # ns > 1 is monotone in K: bisect for the last one-launch K
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if split(mid)[1] > 1 else (mid, hi)
    K = hi if chunks == 1 else hi + 2
    shape = (K, rows) if trans else (rows, K)
    ks, ns = split(K)
    assert ns > 1 and ks >= chunks * (256 if trans else 1024), (shape, ks, ns)
    return shape


SPLITS = [(False, 4, 1), (True, 4, 1), (False, 2, 2), (True, 1, 2)]   # (trans, bits, chunks per range at least)


def _lin(p, trans, xc, xbits, bias=None, act=None, out_codes=False, skinny=True):
    from admmq import packed_linear_int
    return packed_linear_int(_xq(xc, xbits), p, bias, trans, act, out_codes, skinny=skinny)


def _ref(p, a0, trans, xc, xbits, bias):
    return _oracle_layout(a0.T if trans else a0, xc.cpu().numpy(), 1, p.scale, xbits, XMN, XRNG, bias)


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("bits,scheme", [(b, s) for b in range(1, 9) for s in (MSE, SYM, AFF)])
def test_every_width_scheme_and_orientation_bit_for_bit(bits, scheme, trans):
    p, a0 = _weight(SMALL[trans], bits, scheme)
    M, K = (a0.T if trans else a0).shape
    bias = _randn((M,), 700 + M)
    for xbits in (2, 8):
        for N in (1, 3, 8):
            xc = _codes((N, K), xbits, 710 + 3 * N + xbits)
            for b in (None, bias):
                y = _lin(p, trans, xc, xbits, b)
                assert y.dtype == torch.float32 and tuple(y.shape) == (N, M)
                assert _bits_equal(y, _ref(p, a0, trans, xc, xbits, b)), (xbits, N, b is not None)
                assert torch.equal(y, _lin(p, trans, xc, xbits, b, skinny=False)), (xbits, N, b is not None)


@pytest.mark.parametrize("trans,bits,chunks", SPLITS)
def test_k_split_equals_the_oracle(trans, bits, chunks):
    shape = _split_shape(trans, bits, 3 if not trans else 5, chunks)
    p, a0 = _weight(shape, bits, MSE)
    M, K, _, ns = _plan(p, trans)
    assert ns > 1
    bias = _randn((M,), 720)
    for N in (1, 5):
        xc = _codes((N, K), 8, 721 + N)
        for b in (None, bias):
            assert _bits_equal(_lin(p, trans, xc, 8, b), _ref(p, a0, trans, xc, 8, b)), (shape, N, b is not None)


@pytest.mark.parametrize("trans", [False, True])
def test_the_sums_limit(trans):
    """K = 65536, 8-bit codes 255 in one row of W and 0 in the other, ux = 255: U = 255 * 255 * 65536 is the
    largest sum a uint32 holds here; off Sx is taken off in int64. K = 65537 is refused."""
    from admmq import PackedTensor
    K = 65536
    u = torch.tensor([255, 0], dtype=torch.uint8).repeat(K) if trans else torch.tensor([255, 0], dtype=torch.uint8).repeat_interleave(K)
    p = PackedTensor(codes=u.to(DEV), shape=(K, 2) if trans else (2, K), bits=8, qscheme=SYM, scale=float(np.float32(0.013)),
                     zero_point=0, mn=0.0, rng=0.0, index=-1)
    a = np.repeat(np.array([[127], [-128]], dtype=np.int64), K, axis=1)
    xc = torch.full((2, K), 255, dtype=torch.uint8, device=DEV)
    bias = _randn((2,), 730)
    ref = _oracle_layout(a, xc.cpu().numpy(), 1, p.scale, 8, XMN, XRNG, bias)
    assert _plan(p, trans)[3] > 1
    assert _bits_equal(_lin(p, trans, xc, 8, bias), ref)
    big = PackedTensor(codes=torch.zeros(2 * (K + 1), dtype=torch.uint8, device=DEV), shape=(K + 1, 2) if trans else (2, K + 1),
                       bits=8, qscheme=SYM, scale=0.5, zero_point=0, mn=0.0, rng=0.0, index=-1)
    with pytest.raises(ValueError, match="65536"):
        _lin(big, trans, torch.zeros((1, K + 1), dtype=torch.uint8, device=DEV), 8)


def _form_cases():
    return [(False, 4, 0), (True, 4, 0), (False, 4, 1), (True, 4, 1)]   # (trans, bits, 0: one launch / 1: split)


def _form_weight(trans, bits, split):
    shape = _split_shape(trans, bits, 37, 1) if split else SMALL[trans]
    p, a0 = _weight(shape, bits, MSE)
    assert (_plan(p, trans)[3] > 1) == bool(split)
    return p, a0


@pytest.mark.parametrize("trans,bits,split", _form_cases())
def test_output_forms_equal_the_quantizers_of_the_float_output(trans, bits, split):
    from admmq import act_encode, fixed_quantize
    p, a0 = _form_weight(trans, bits, split)
    M, K = _plan(p, trans)[:2]
    xc, bias = _codes((8, K), 5, 740), _randn((M,), 741)
    y = _lin(p, trans, xc, 5, bias)
    lo, hi = float(y.quantile(0.2)), float(y.quantile(0.8))   # some outputs clamp, not all
    for obits in (3, 8):
        act = (obits, lo, hi)
        want = act_encode(y, act, check=False)
        assert torch.equal(_lin(p, trans, xc, 5, bias, act), fixed_quantize(y, obits, want.mn, want.rng))
        got = _lin(p, trans, xc, 5, bias, act, out_codes=True)
        assert 0 < int(want.clamped) < y.numel()
        assert torch.equal(got.codes, want.codes) and int(got.clamped) == int(want.clamped)
        assert int(_lin(p, trans, xc, 5, bias, act, out_codes=True).clamped) == int(want.clamped)   # zeroed per call


@pytest.mark.parametrize("trans,bits,split", _form_cases())
def test_row_c_of_eight_is_the_call_on_that_row(trans, bits, split):
    p, _ = _form_weight(trans, bits, split)
    M, K = _plan(p, trans)[:2]
    xc, bias = _codes((8, K), 8, 750), _randn((M,), 751)
    y8 = _lin(p, trans, xc, 8, bias)
    for c in range(8):
        assert torch.equal(_lin(p, trans, xc[c:c + 1].contiguous(), 8, bias)[0], y8[c]), c


@pytest.mark.parametrize("trans,split,out_codes", [(False, 0, False), (True, 1, True), (False, 1, False), (True, 0, True)])
def test_nothing_else_is_written(trans, split, out_codes):
    """Guard bands round y / y_codes, the counter, the workspace and the code stream (no stream here ends on a dword);
    x starts one byte past a 16-byte boundary."""
    from admmq import _lib, packed_rowsums
    from admmq.packed import _meta_words
    p, _ = _form_weight(trans, 4, split)
    M, K = _plan(p, trans)[:2]
    lib, meta = _lib.load(), _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    need = lib.admmq_packed_igemv_workspace_size(ctypes.byref(meta), 1 if trans else 0, M, K, 8)
    assert (need > 0) == bool(split)
    xc, bias = _codes((8, K), 8, 760), _randn((M,), 761)
    act = (6, -2.0, 2.0)
    ref = _lin(p, trans, xc, 8, bias, act if out_codes else None, out_codes)
    xo = torch.empty(8 * K + 32, dtype=torch.uint8, device=DEV)
    xo = xo[(16 - xo.data_ptr() % 16) % 16 + 1:][:8 * K]
    xo.copy_(xc.reshape(-1))
    nbytes = p.codes.numel()
    for fill in (0x00, 0xFF):
        cbuf = torch.full((64 + nbytes + 512,), fill, dtype=torch.uint8, device=DEV)
        cbuf[64:64 + nbytes].copy_(p.codes)
        assert cbuf[64:].data_ptr() % 16 == 0
        ybuf = torch.full((8 * M + 128,), 77, dtype=torch.uint8 if out_codes else torch.float32, device=DEV)
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        cl = torch.full((3,), -9, dtype=torch.int32, device=DEV)
        xq, oq = _lib.ActQ(8, 1, XMN, XRNG), _lib.ActQ(act[0], 1, act[1], act[2] - act[1])
        rc = lib.admmq_packed_igemv(_lib.ptr(cbuf[64:]), ctypes.byref(meta), 1 if trans else 0, M, K, _lib.ptr(xo),
                                    ctypes.byref(xq), _lib.ptr(packed_rowsums(p, trans)), 8, _lib.ptr(bias),
                                    _lib.ptr(None if out_codes else ybuf[64:]), _lib.ptr(ybuf[64:] if out_codes else None),
                                    ctypes.byref(oq) if out_codes else None, _lib.ptr(cl[1:] if out_codes else None),
                                    _lib.ptr(ws), need, _lib.stream_handle(DEV))
        assert rc == 0, lib.admmq_last_error()
        torch.cuda.synchronize()
        assert bool((ybuf[:64] == 77).all()) and bool((ybuf[64 + 8 * M:] == 77).all())
        assert bool((ws[need:] == 0xA5).all()) and int(cl[0]) == -9 and int(cl[2]) == -9
        assert bool((cbuf[:64] == fill).all()) and bool((cbuf[64 + nbytes:] == fill).all())
        out = ybuf[64:64 + 8 * M].view(8, M)
        if out_codes:
            assert torch.equal(out, ref.codes) and int(cl[1]) == int(ref.clamped)
        else:
            assert torch.equal(out, ref)


def test_skinny_routes_by_rows_and_the_two_routes_agree(monkeypatch):
    from admmq import export, packed
    p, _ = _weight(SMALL[False], 4, MSE)
    K = SMALL[False][1]
    calls = []
    for name in ("_igemv", "_igemm"):
        monkeypatch.setattr(packed, name, lambda *a, _f=getattr(packed, name), _n=name: (calls.append(_n), _f(*a))[1])
    x8, x9 = _codes((2, 4, K), 8, 770), _codes((9, K), 8, 771)
    y8, y9 = _lin(p, False, x8, 8), _lin(p, False, x9, 8)
    assert calls == ["_igemv", "_igemm"] and tuple(y8.shape) == (2, 4, 33)
    assert torch.equal(y8, _lin(p, False, x8, 8, skinny=False)) and torch.equal(y9, _lin(p, False, x9, 8, skinny=False))
    assert calls == ["_igemv", "_igemm", "_igemm", "_igemm"]

    fout, fin, R = 70, 64, 24
    pf = _factors([(fout, R), (fin, R)], 40)
    layer = export.build_cpfc_layer(R, pf, _randn((fout,), 41), fin, fout, act_quant=[(6, -1.0, 1.0), None], integer=True,
                                    in_act=(8, -4.0, 4.0))
    assert layer.skinny is False and "skinny" not in repr(layer) and "skinny" not in layer.get_extra_state()
    for shape in [(1, fin), (2, 4, fin), (9, fin)]:
        x = _randn(shape, 772).clamp_(-3.9, 3.9)
        layer.skinny = False
        want = layer(x)
        layer.skinny = True
        assert torch.equal(layer(x), want) and "skinny=True" in repr(layer)
