"""Integer packed GEMM on the MI355X: activation codes round-trip to
fixed_quantize's bits and count their clamps, k_packed_igemm equals the numpy oracle (int64
sums, then the double formula) bit for bit for every weight width, scheme, orientation, layout
and regime - which is also the check of the i8 MFMA's operand lanes, on asymmetric random codes -
its results do not depend on the call or the batch, a codes output equals act_encode of the float
output, nothing outside the outputs / the workspace is written, and the 2-way integer layers
equal the chain of functional calls."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from torch import nn

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE, MINMAX, SYM, AFF = "tensor_mseminmax_symmetric", "tensor_minmax", "tensor_symmetric", "tensor_affine"
DEV = torch.device("cuda:0")
XMN, XRNG = float(np.float32(-0.7)), float(np.float32(2.3))   # the activation codes' range: mn != 0


def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _codes(shape, bits, seed):
    """Asymmetric random activation codes 0 .. 2^bits - 1 (uint8, on the device)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1 << bits, shape, generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)


def _xq(codes, bits, mn=XMN, rng=XRNG):
    from admmq import QuantizedActivation
    return QuantizedActivation(codes, bits, mn, rng)


# 8-bit affine: a = (u - 128) - zp fits int8 only for zp = 0; this range gives trunc(tmin / scale) = -128
AFF8_OK = dict(tmin=-128.4 / 255 * 2, tmax=126.6 / 255 * 2)


@functools.lru_cache(maxsize=None)
def _packed(shape, bits, scheme, seed=7, kw=()):
    """(PackedTensor of a random tensor, its integer weight a = (u - q) - zp as int64 numpy) - made once."""
    from admmq import quantize_packed
    p = quantize_packed([_randn(shape, seed + 131 * bits + shape[0], 0.3)], bits, scheme, **dict(kw))[0]
    zp = p.zero_point if scheme == AFF else 0
    a = p.levels().cpu().numpy().astype(np.int64) - (1 << (bits - 1)) - zp
    return p, a


def _weight(shape, bits, scheme):
    if scheme == AFF and bits == 8:
        return _packed(shape, bits, scheme, kw=tuple(AFF8_OK.items()))
    return _packed(shape, bits, scheme)


def _oracle(a, ux_kc, scale, xbits, mn, rng, bias):
    """[M, C] float32: int64 sums, then the contract's double formula, one rounding to float32."""
    S = a @ ux_kc.astype(np.int64)
    A = a.sum(axis=1)
    g = np.float64(np.float32(rng)) / np.float64((1 << xbits) - 1)
    v = np.float64(np.float32(scale)) * (g * S.astype(np.float64) + np.float64(np.float32(mn)) * A.astype(np.float64)[:, None])
    if bias is not None:
        v = v + bias.astype(np.float64)[:, None]
    return v.astype(np.float32)


def _oracle_layout(a, x, layout, scale, xbits, mn, rng, bias):
    """The oracle in the output's layout; x: numpy codes [nb, K, N] (layout 0) or [T, K] (layout 1)."""
    b = None if bias is None else bias.cpu().numpy()
    if layout == 0:
        nb, K, N = x.shape
        y = _oracle(a, x.transpose(1, 0, 2).reshape(K, nb * N), scale, xbits, mn, rng, b)
        return np.ascontiguousarray(y.reshape(-1, nb, N).transpose(1, 0, 2))
    return np.ascontiguousarray(_oracle(a, x.T, scale, xbits, mn, rng, b).T)


def _run(p, trans, xq, layout, bias=None, act=None, out_codes=False):
    from admmq import packed_linear_int, packed_rowsums
    from admmq.packed import _meta_words, _weight_dims, packed_igemm
    if layout == 0:   # x [nb, K, N]
        M, K = _weight_dims(p, trans)
        return packed_igemm(p.codes, _meta_words(p), trans, M, K, xq, packed_rowsums(p, trans), 0, bias, act, out_codes)
    return packed_linear_int(xq, p, bias, trans, act, out_codes)


def _bits_equal(y, ref):
    return torch.equal(y.cpu().view(torch.int32), torch.from_numpy(ref).view(torch.int32))


# ------------------------------------------------------------------ encode and decode
def _np_levels(x, bits, mn, rng):
    """numpy float32 restatement of the contract's r and qi."""
    n = np.float32((1 << bits) - 1)
    with np.errstate(all="ignore"):
        r = (x - np.float32(mn)) / np.float32(rng)
        return np.floor(r * n + np.float32(0.5)), n


@pytest.mark.parametrize("bits", range(2, 9))
def test_codes_round_trip_to_fixed_quantize(bits):
    """A range that covers the data: decode(encode(x)) has fixed_quantize's bits, nothing is clamped.
    Sizes 1, 3, 4099 (scalar head and tail around the 16-byte vectors)."""
    from admmq import act_encode, fixed_quantize
    for numel in (1, 3, 4099):
        x = _randn((numel,), 100 + bits).clamp_(-3.9, 3.9)
        q = act_encode(x, (bits, -4.0, 4.0))
        assert q.codes.dtype == torch.uint8 and q.codes.shape == x.shape and int(q.clamped) == 0
        fq = fixed_quantize(x, bits, q.mn, q.rng)
        assert torch.equal(q.dequantize().view(torch.int32), fq.view(torch.int32)), (bits, numel)
        qi, n = _np_levels(x.cpu().numpy(), bits, q.mn, q.rng)
        assert np.array_equal(q.codes.cpu().numpy(), qi.astype(np.uint8))


@pytest.mark.parametrize("bits", [2, 5, 8])
def test_clamped_elements_saturate_and_are_counted(bits):
    from admmq import act_encode
    x = _randn((4099,), 120 + bits, 3.0)
    x[7] = float("nan")
    x[11], x[12] = 1e9, -1e9
    q = act_encode(x, (bits, -2.0, 2.0), check=False)
    qi, n = _np_levels(x.cpu().numpy(), bits, q.mn, q.rng)
    bad = ~((qi >= 0) & (qi <= n))
    assert bad.sum() > 100 and bad[7]
    want = np.where(np.isnan(qi), 0, np.clip(qi, 0, n)).astype(np.uint8)
    got = q.codes.cpu().numpy()
    assert np.array_equal(got, want)
    assert got[7] == 0 and got[11] == int(n) and got[12] == 0
    assert int(q.clamped) == int(bad.sum())
    with pytest.raises(ValueError, match="clamped"):
        act_encode(x, (bits, -2.0, 2.0))


@pytest.mark.parametrize("off", [1, 4])
def test_misaligned_views(off):
    """Codes `off` bytes, floats 4 bytes past a 16-byte boundary: the same codes and values."""
    from admmq import act_decode, act_encode
    from admmq import _lib
    x = _randn((4099,), 140).clamp_(-3.9, 3.9)
    ref = act_encode(x, (5, -4.0, 4.0))
    xo = torch.empty(4099 + 1, device=DEV)[1:]
    xo.copy_(x)
    co = torch.full((4099 + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    cv = co[off:off + 4099]
    assert xo.data_ptr() % 16 == 4 and cv.data_ptr() % 16 == off
    q = _lib.ActQ(5, 1, ref.mn, ref.rng)
    cnt = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    assert lib.admmq_act_encode(_lib.ptr(xo), _lib.ptr(cv), 4099, ctypes.byref(q), _lib.ptr(cnt),
                                _lib.stream_handle(DEV)) == 0, lib.admmq_last_error()
    assert torch.equal(cv, ref.codes) and int(cnt) == 0
    assert bool((co[:off] == 0xEE).all()) and bool((co[off + 4099:] == 0xEE).all())
    yo = torch.full((4099 + 8,), -5.5, device=DEV)
    yv = yo[1:1 + 4099]
    assert lib.admmq_act_decode(_lib.ptr(cv), _lib.ptr(yv), 4099, ctypes.byref(q), _lib.stream_handle(DEV)) == 0
    assert torch.equal(yv, act_decode(ref.codes, 5, ref.mn, ref.rng))
    assert float(yo[0]) == -5.5 and bool((yo[1 + 4099:] == -5.5).all())


# ------------------------------------------------------------------------- exactness
SHAPES = [(64, 134), (134, 9), (33, 65), (1, 7)]


def test_row_sums_equal_the_integer_weight_sums():
    from admmq import packed_rowsums
    for bits, scheme in [(1, MSE), (3, AFF), (5, SYM), (8, AFF), (8, MSE)]:
        for shape in SHAPES + [(70, 1141)]:
            p, a = _weight(shape, bits, scheme)
            for trans in (False, True):
                A = packed_rowsums(p, trans)
                assert A.dtype == torch.int32
                assert np.array_equal(A.cpu().numpy(), (a.T if trans else a).sum(axis=1)), (bits, scheme, shape, trans)
                assert packed_rowsums(p, trans) is A   # kept on the packed tensor


@pytest.mark.parametrize("bits,scheme", [(b, s) for b in range(1, 9) for s in (MSE, SYM, AFF)])
def test_equals_the_integer_oracle_bit_for_bit(bits, scheme):
    """Every weight width and scheme x activation bits {2, 5, 8} x four packed shapes in both
    orientations x columns {1, 49, 65} with nb {1, 3} (layout 0) and {1, 16, 65} tokens (layout 1),
    with and without a bias: torch.equal to the oracle. An operand lane of the i8 MFMA taken
    from the wrong k, row or column changes these sums."""
    cases = [(0, n, nb) for n in (1, 49, 65) for nb in (1, 3)] + [(1, t, 1) for t in (1, 16, 65)]
    ncalls = 0
    for shape in SHAPES:
        p, a0 = _weight(shape, bits, scheme)
        for trans in (False, True):
            a = a0.T if trans else a0
            M, K = a.shape
            bias = _randn((M,), 200 + M)
            for xbits in (2, 5, 8):
                for layout, n, nb in cases:
                    xc = _codes((nb, K, n) if layout == 0 else (n, K), xbits, 300 + 7 * n + nb + xbits)
                    xnp = xc.cpu().numpy()
                    for b in (None, bias):
                        y = _run(p, trans, _xq(xc, xbits), layout, b)
                        ref = _oracle_layout(a, xnp, layout, p.scale, xbits, XMN, XRNG, b)
                        assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape
                        assert _bits_equal(y, ref), (shape, trans, xbits, layout, n, nb, b is not None)
                        ncalls += 1
    assert ncalls == len(SHAPES) * 2 * 3 * len(cases) * 2


def test_affine_record_outside_int8_is_refused():
    from admmq import packed_linear_int, packed_rowsums
    p, _ = _packed((33, 65), 8, AFF, kw=(("tmin", -0.2), ("tmax", 1.0)))
    assert p.zero_point != 0
    with pytest.raises(ValueError, match="int8"):
        packed_linear_int(_xq(_codes((3, 65), 4, 1), 4), p)
    with pytest.raises(ValueError, match="int8"):
        packed_rowsums(p)
    pm, _ = _packed((33, 65), 4, MINMAX)
    with pytest.raises(ValueError, match="tensor_minmax"):
        packed_linear_int(_xq(_codes((3, 65), 4, 1), 4), pm)


def _raw(p, trans, x, xbits, layout, N, nb, bias, y=None, y_codes=None, out=None, codes=None, ws=None, clamped=None,
         rowsums=None):
    """admmq_packed_igemm through ctypes on caller-owned buffers; returns the workspace bytes needed."""
    from admmq import _lib, packed_rowsums
    from admmq.packed import _meta_words, _weight_dims
    lib = _lib.load()
    M, K = _weight_dims(p, trans)
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    need = lib.admmq_packed_igemm_workspace_size(M, K, N, nb)
    if ws is None:
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    xq = _lib.ActQ(xbits, 1, XMN, XRNG)
    oq = None if out is None else _lib.ActQ(out[0], 1, out[1], out[2])
    rs = packed_rowsums(p, trans) if rowsums is None else rowsums
    rc = lib.admmq_packed_igemm(_lib.ptr(p.codes if codes is None else codes), ctypes.byref(meta), 1 if trans else 0, M, K,
                                _lib.ptr(x), ctypes.byref(xq), _lib.ptr(rs), layout, N, nb, _lib.ptr(bias), _lib.ptr(y),
                                _lib.ptr(y_codes), ctypes.byref(oq) if oq is not None else None, _lib.ptr(clamped),
                                _lib.ptr(ws), ws.numel(), _lib.stream_handle(DEV))
    assert rc == 0, lib.admmq_last_error()
    torch.cuda.synchronize()
    return need


@pytest.mark.parametrize("shape,trans,N,nb,parallel", [((64, 4097), False, 5, 1, True), ((64, 134), False, 257, 64, False),
                                                       ((4097, 70), True, 3, 2, True)])
def test_both_regimes_equal_the_oracle_and_the_caller_workspace_route(shape, trans, N, nb, parallel):
    """K = 4097 with few tiles: many K pieces as separate workgroups + k_packed_ireduce; nb N = 64 * 257:
    >= 256 tiles, one workgroup per tile over all of K. The op route and admmq_packed_igemm on a
    caller's workspace both equal the oracle."""
    from admmq import _lib
    p, a0 = _weight(shape, 4, MSE)
    a = a0.T if trans else a0
    M, K = a.shape
    need = _lib.load().admmq_packed_igemm_workspace_size(M, K, N, nb)
    assert (need > 0) == parallel
    xc = _codes((nb, K, N), 8, 400 + K)
    bias = _randn((M,), 401)
    ref = _oracle_layout(a, xc.cpu().numpy(), 0, p.scale, 8, XMN, XRNG, bias)
    y = _run(p, trans, _xq(xc, 8), 0, bias)
    assert _bits_equal(y, ref)
    yr = torch.empty_like(y)
    _raw(p, trans, xc, 8, 0, N, nb, bias, y=yr)
    assert torch.equal(yr, y)


# ---------------------------------------------------------------------- independence
@pytest.mark.parametrize("shape,trans,N", [((64, 134), False, 49), ((64, 4097), False, 4), ((134, 64), True, 70)])
def test_calls_repeat_and_images_do_not_depend_on_the_batch(shape, trans, N):
    p, a0 = _weight(shape, 4, MSE)
    K = a0.shape[0] if trans else a0.shape[1]
    xc = _codes((3, K, N), 5, 500 + N)
    y1 = _run(p, trans, _xq(xc, 5), 0)
    assert torch.equal(y1, _run(p, trans, _xq(xc, 5), 0))
    for b in range(3):
        assert torch.equal(_run(p, trans, _xq(xc[b:b + 1].contiguous(), 5), 0)[0], y1[b]), b
    xl = _codes((5, K), 5, 501)
    yl = _run(p, trans, _xq(xl, 5), 1)
    assert torch.equal(yl, _run(p, trans, _xq(xl, 5), 1))
    assert torch.equal(_run(p, trans, _xq(xl[2:3].contiguous(), 5), 1)[0], yl[2])


# ---------------------------------------------------------------------- codes output
@pytest.mark.parametrize("shape,trans,layout,n,nb", [((64, 134), False, 0, 49, 3), ((134, 9), True, 1, 65, 1),
                                                     ((64, 4097), False, 0, 5, 1), ((33, 65), False, 1, 16, 1)])
def test_codes_output_equals_act_encode_of_the_float_output(shape, trans, layout, n, nb):
    from admmq import act_encode, fixed_quantize
    p, a0 = _weight(shape, 4, MSE)
    a = a0.T if trans else a0
    M, K = a.shape
    xc = _codes((nb, K, n) if layout == 0 else (n, K), 5, 600 + n)
    bias = _randn((M,), 601)
    y = _run(p, trans, _xq(xc, 5), layout, bias)
    lo, hi = float(y.min()), float(y.max())
    for obits, act in [(4, (4, lo - 0.1, hi + 0.1)), (8, (8, lo - 0.1, hi + 0.1)), (3, (3, 0.25 * lo, 0.25 * hi))]:
        want = act_encode(y, act, check=False)
        got = _run(p, trans, _xq(xc, 5), layout, bias, act, out_codes=True)
        assert got.codes.dtype == torch.uint8 and got.codes.shape == y.shape
        assert (got.bits, got.mn, got.rng) == (want.bits, want.mn, want.rng)
        assert torch.equal(got.codes, want.codes), (obits,)
        assert int(got.clamped) == int(want.clamped)
        assert (int(got.clamped) > 0) == (obits == 3)
        # the float + quantizer form: fixed_quantize of the float output
        yq = _run(p, trans, _xq(xc, 5), layout, bias, act)
        assert torch.equal(yq.view(torch.int32), fixed_quantize(y, act[0], want.mn, want.rng).view(torch.int32))


def test_two_stage_chain_equals_the_oracle():
    """Stage 1 writes codes, stage 2 reads them: the oracle of the chain (the inter-stage codes are
    the oracle's float32 output pushed through the contract's encode in numpy)."""
    p1, a1 = _weight((64, 134), 4, MSE)      # [K = 64 -> R = 134] as the transpose
    p2, a2 = _weight((70, 134), 5, SYM)      # [M = 70, R = 134]
    xc = _codes((16, 64), 8, 700)
    bias = _randn((70,), 701)
    h_ref = _oracle_layout(a1.T, xc.cpu().numpy(), 1, p1.scale, 8, XMN, XRNG, None)     # [16, 134]
    lo, hi = float(h_ref.min()) - 0.05, float(h_ref.max()) + 0.05
    from admmq.quantization import act_range
    mn, rng = act_range(lo, hi)
    qi, n = _np_levels(h_ref, 6, mn, rng)
    hu = np.clip(qi, 0, n).astype(np.uint8)
    h = _run(p1, True, _xq(xc, 8), 1, None, (6, lo, hi), out_codes=True)
    assert np.array_equal(h.codes.cpu().numpy(), hu) and int(h.clamped) == 0
    y = _run(p2, False, h, 1, bias)
    ref = _oracle_layout(a2, hu, 1, p2.scale, 6, mn, rng, bias)
    assert _bits_equal(y, ref)


# ------------------------------------------------------------ against the float path
@pytest.mark.parametrize("shape,trans,layout,n,nb", [((64, 134), False, 0, 49, 3), ((134, 64), True, 1, 65, 1),
                                                     ((64, 4097), False, 1, 5, 1)])
def test_integer_route_against_the_float_path(shape, trans, layout, n, nb):
    """|Y_int - Yd| <= 2^-22 (|W| (|X| + |G|)) + 2^-23 |Yd| element-wise, Yd the float64 product of the
    de-quantized weight with fixed_quantize(x), G = u rng / n: one float32 rounding of s a and three
    of the activation's de-quantization (2.1 * 2^-24 per product), plus the final rounding."""
    from admmq import act_encode, fixed_quantize
    p, a0 = _weight(shape, 4, MSE)
    D = p.dequantize()
    W = (D.T if trans else D).double().cpu()
    M, K = W.shape
    x = _randn((nb, K, n) if layout == 0 else (n, K), 800 + n).clamp_(-3.9, 3.9)
    xq = act_encode(x, (8, -4.0, 4.0))
    X = fixed_quantize(x, 8, xq.mn, xq.rng).double().cpu()
    G = xq.codes.double().cpu() * float(xq.rng) / 255.0
    y = _run(p, trans, xq, layout).double().cpu()
    if layout == 0:
        yd = torch.einsum("mk,bkn->bmn", W, X)
        mag = torch.einsum("mk,bkn->bmn", W.abs(), X.abs() + G.abs())
    else:
        yd = X @ W.T
        mag = (X.abs() + G.abs()) @ W.abs().T
    bound = 2.0 ** -22 * mag + 2.0 ** -23 * yd.abs()
    err = (y - yd).abs()
    frac = float((err / bound.clamp_min(1e-300)).max())
    print(f"integer vs float path {(shape, trans, layout, n, nb)}: largest fraction of the bound used = {frac:.4f}")
    assert bool((err <= bound).all()), frac


# --------------------------------------------------------------- nothing else is touched
@pytest.mark.parametrize("shape,bits,N,nb,layout", [((33, 65), 3, 70, 1, 0), ((134, 9), 5, 3, 2, 0), ((70, 1141), 3, 4, 1, 0),
                                                    ((33, 65), 3, 17, 1, 1)])
def test_nothing_outside_the_outputs_or_the_workspace_is_touched(shape, bits, N, nb, layout):
    """Guard bytes around y / y_codes, behind the workspace and around the code stream (filled 0x00
    and 0xFF); x codes at an odd address and bias 4 bytes past a 16-byte boundary."""
    from admmq import _lib
    from admmq.packed import packed_bytes
    p, a0 = _weight(shape, bits, SYM)
    nbytes = packed_bytes(shape[0] * shape[1], bits)
    assert p.codes.numel() == nbytes
    for trans in (False, True):
        a = a0.T if trans else a0
        M, K = a.shape
        xc = _codes((nb, K, N) if layout == 0 else (N, K), 8, 900 + N)
        xbuf = torch.full((xc.numel() + 32,), 0x5A, dtype=torch.uint8, device=DEV)
        xo = xbuf[1:1 + xc.numel()]
        xo.copy_(xc.reshape(-1))
        bias = _randn((M,), 901)
        bo = torch.empty(M + 1, device=DEV)[1:]
        bo.copy_(bias)
        assert xo.data_ptr() % 2 == 1 and bo.data_ptr() % 16 == 4
        total = nb * M * N
        ref = _oracle_layout(a, xc.cpu().numpy(), layout, p.scale, 8, XMN, XRNG, bias)
        act = (6, float(ref.min()) - 0.1, float(ref.max()) + 0.1)
        from admmq.quantization import act_range
        mn, rng = act_range(act[1], act[2])
        want_codes = _run(p, trans, _xq(xc, 8), layout, bias, act, out_codes=True).codes
        for fill in (0x00, 0xFF):
            cbuf = torch.full((64 + nbytes + 512,), fill, dtype=torch.uint8, device=DEV)
            cview = cbuf[64:64 + nbytes]
            cview.copy_(p.codes)
            need = _lib.load().admmq_packed_igemm_workspace_size(M, K, N, nb)
            ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
            ybuf = torch.full((total + 128,), -12345.5, device=DEV)
            _raw(p, trans, xo, 8, layout, N, nb, bo, y=ybuf[64:64 + total], codes=cview, ws=ws)
            assert bool((ybuf[:64] == -12345.5).all()) and bool((ybuf[64 + total:] == -12345.5).all())
            assert _bits_equal(ybuf[64:64 + total].view(ref.shape), ref)
            ycb = torch.full((total + 128,), 0xC3, dtype=torch.uint8, device=DEV)
            cnt = torch.full((3,), 99, dtype=torch.int32, device=DEV)
            _raw(p, trans, xo, 8, layout, N, nb, bo, y_codes=ycb[61:61 + total], out=(6, mn, rng), codes=cview, ws=ws,
                 clamped=cnt[1:2])
            assert bool((ycb[:61] == 0xC3).all()) and bool((ycb[61 + total:] == 0xC3).all())
            assert torch.equal(ycb[61:61 + total].view(want_codes.shape), want_codes)
            assert cnt.tolist() == [99, 0, 99]
            assert bool((ws[need:] == 0xA5).all())
            assert bool((cbuf[:64] == fill).all()) and bool((cbuf[64 + nbytes:] == fill).all())
            assert bool((xbuf[:1] == 0x5A).all()) and bool((xbuf[1 + xc.numel():] == 0x5A).all())


# ----------------------------------------------------------------------------- layers
def _factors(shapes, seed, bits=4):
    from admmq import quantize_packed
    return quantize_packed([_randn(s, seed + i, 0.3) for i, s in enumerate(shapes)], bits, MSE)


def _rel(y, ref):
    return float((y.double() - ref.double()).norm() / ref.double().norm())


def _layer_checks(build, functional, x, in_act, tmp_path, fresh_factors):
    """build(factors=None, **kw) -> module; functional(x) -> the chain of functional calls."""
    from admmq import fixed_quantize
    from admmq.quantization import act_range
    plain = build()                                        # the float packed layer, no quantizers
    with torch.no_grad():
        y_plain = plain(x)
        first = next(plain.children())
        h = first(x)                                       # stage 1's float output: the inter-stage range
    mid = (6, float(h.min()) - 0.05, float(h.max()) + 0.05)
    out = (8, float(y_plain.min()) - 0.05, float(y_plain.max()) + 0.05)
    acts = [mid, out]
    layer = build(act_quant=acts, integer=True, in_act=in_act)
    with torch.no_grad():
        y = layer(x)
        assert y.dtype == torch.float32 and y.shape == y_plain.shape
        assert torch.equal(y.view(torch.int32), functional(x, acts).view(torch.int32))
        assert [int(c) for c in layer.last_clamped] == [0, 0]
        # state dict -> file -> a fresh layer built from other factors and quantizers
        path = str(tmp_path / "int_layer.pt")
        torch.save(layer.state_dict(), path)
        fresh = build(factors=fresh_factors, act_quant=[(5, -1.0, 1.0), None], integer=True, in_act=(4, -1.0, 1.0))
        assert not torch.equal(fresh(x), y)
        fresh.load_state_dict(torch.load(path, map_location=DEV, weights_only=True))
        assert torch.equal(fresh(x), y)
        # rounding differences sit under the quantization noise
        mn, rng = act_range(in_act[1], in_act[2])
        fl = build(act_quant=acts)
        y_fl = fl(fixed_quantize(x, in_act[0], mn, rng))
        d_int, d_q = _rel(y, y_fl), _rel(y_fl, y_plain)
        print(f"integer layer vs float packed layer with quantizers: {d_int:.3e}; that layer vs unquantized: {d_q:.3e}")
        assert d_int < d_q
        # compiled module containing the integer layer
        seq = nn.Sequential(layer)
        assert torch.equal(torch.compile(seq)(x), y)


def test_cpfc_integer_layer(tmp_path):
    from admmq import act_encode, export, packed_linear_int
    fout, fin, R = 70, 64, 24
    pf = _factors([(fout, R), (fin, R)], 40)      # [B, A]
    bias = _randn((fout,), 41)
    x = _randn((3, 5, fin), 42).clamp_(-3.9, 3.9)
    in_act = (8, -4.0, 4.0)

    def build(factors=None, **kw):
        return export.build_cpfc_layer(R, pf if factors is None else factors, bias, fin, fout, **kw)

    def functional(x, acts):
        xq = act_encode(x, in_act)
        h = packed_linear_int(xq, pf[1], None, True, acts[0], out_codes=True)
        return packed_linear_int(h, pf[0], bias, False, acts[1])

    layer = build(act_quant=[(6, -1.0, 1.0), None], integer=True, in_act=in_act)
    assert type(layer) is export.IntegerPackedPair and [n for n, _ in layer.named_children()] == ["fc1", "fc2"]
    assert type(build()) is nn.Sequential       # the default arguments build today's module
    _layer_checks(build, functional, x, in_act, tmp_path, _factors([(fout, R), (fin, R)], 78))


def test_cp2conv_integer_layer(tmp_path):
    from admmq import act_encode, export, packed_conv1x1_int
    cout, cin, R, stride = 128, 64, 40, 2
    pf = _factors([(cout, R), (cin, R)], 30)      # [A, B]
    bias = _randn((cout,), 31)
    x = _randn((2, cin, 9, 9), 32).clamp_(-3.9, 3.9)
    in_act = (8, -4.0, 4.0)

    def build(factors=None, **kw):
        return export.build_cp2conv_layer(R, pf if factors is None else factors, bias, cin, cout, 0, stride, **kw)

    def functional(x, acts):
        xq = act_encode(x, in_act)
        h = packed_conv1x1_int(xq, pf[1], None, True, stride, acts[0], out_codes=True)
        return packed_conv1x1_int(h, pf[0], bias, False, 1, acts[1])

    layer = build(act_quant=[(6, -1.0, 1.0), None], integer=True, in_act=in_act)
    assert type(layer) is export.IntegerPackedPair and [n for n, _ in layer.named_children()] == ["conv1", "conv2"]
    _layer_checks(build, functional, x, in_act, tmp_path, _factors([(cout, R), (cin, R)], 79))


def test_meta_shapes_and_inference_only():
    from admmq import _lib, act_encode
    from admmq.packed import _meta_words
    ops = _lib.ops()
    m = torch.device("meta")
    p, _ = _weight((64, 134), 4, MSE)
    w = _meta_words(p)
    y, c = ops.packed_igemm(p.codes.to(m), w, False, 64, 134, torch.empty(3, 134, 7, 5, dtype=torch.uint8, device=m), 8,
                            0.0, 1.0, torch.empty(64, dtype=torch.int32, device=m), 0, None, 0, 0.0, 0.0, False)
    assert tuple(y.shape) == (3, 64, 7, 5) and y.dtype == torch.float32 and c.numel() == 0
    y, c = ops.packed_igemm(p.codes.to(m), w, True, 134, 64, torch.empty(5, 64, dtype=torch.uint8, device=m), 8, 0.0, 1.0,
                            torch.empty(134, dtype=torch.int32, device=m), 1, None, 4, 0.0, 1.0, True)
    assert tuple(y.shape) == (5, 134) and y.dtype == torch.uint8 and tuple(c.shape) == (1,)
    x = _randn((3, 134), 50).requires_grad_()
    with pytest.raises(RuntimeError, match="inference only"):
        act_encode(x, (8, -4.0, 4.0))
    with pytest.raises(RuntimeError, match="inference only"):
        ops.act_encode(x, 8, -4.0, 8.0)
    with torch.no_grad():
        assert int(act_encode(x.clamp(-3.9, 3.9), (8, -4.0, 4.0)).clamped) == 0


def test_ctypes_route_equals_the_op_route(monkeypatch):
    """The route the Python functions take when ADMMQ_LIB selects another build of the library (no
    ops library): the same bits as torch.ops.admmq, for codes, values, row sums, float and codes outputs."""
    from admmq import _lib, act_decode, act_encode, packed_rowsums
    from admmq.packed import _meta_words, _rowsums
    p, a0 = _weight((64, 134), 4, MSE)
    x = _randn((3, 134), 1000).clamp_(-3.9, 3.9)
    bias = _randn((64,), 1001)
    xc = _codes((2, 134, 49), 5, 1002)

    def run():
        xq = act_encode(x, (8, -4.0, 4.0))
        y = _run(p, False, xq, 1, bias)
        h = _run(p, False, xq, 1, bias, (6, float(y.min()) + 0.3, float(y.max()) + 0.1), out_codes=True)
        return (xq.codes, xq.clamped, act_decode(xq.codes, 8, xq.mn, xq.rng), _rowsums(p.codes, _meta_words(p), True, 134, 64),
                y, h.codes, h.clamped, _run(p, False, _xq(xc, 5), 0, None, (4, -2.0, 2.0)))

    ops = run()
    monkeypatch.setattr(_lib, "use_ops", lambda: False)
    raw = run()
    assert int(ops[6]) > 0
    for i, (o, r) in enumerate(zip(ops, raw)):
        assert o.dtype == r.dtype and torch.equal(o.view(torch.uint8) if o.dtype == torch.float32 else o,
                                                  r.view(torch.uint8) if r.dtype == torch.float32 else r), i
    assert np.array_equal(packed_rowsums(p, True).cpu().numpy(), a0.T.sum(axis=1))
