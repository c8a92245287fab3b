"""Half-precision packed GEMM on the MI355X: k_packed_hgemm on bf16 / fp16
activations decodes exactly dequantize_packed's weight (identity activations: bit-exact, the
tensor_minmax column sum included), its float32 result meets a derived forward bound against
float64, the half result is one round-to-nearest-even conversion of the float32 one, the bits do
not depend on the call, the batch or the regime, nothing outside the stream / the output / the
workspace is touched, and the packed layers run on half inputs before and after .half()."""
import ctypes
import functools

import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE, MINMAX, SYM, AFF = "tensor_mseminmax_symmetric", "tensor_minmax", "tensor_symmetric", "tensor_affine"
SCHEMES = [MSE, MINMAX, SYM, AFF]
DTYPES = [torch.bfloat16, torch.float16]
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # unit roundoff of one conversion to the type
DEV = torch.device("cuda:0")
ULP = 2.0 ** -23   # one full float32 ulp per operation (the MFMA's internal adds are not documented as RNE)


def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _hx(shape, seed, dtype):
    """randn rounded to dtype, |x| < 2^-8 replaced by +-2^-8: no half subnormals (nor products near them)."""
    x = _randn(shape, seed).to(dtype)
    tiny = torch.where(x < 0, -(2.0 ** -8), 2.0 ** -8).to(dtype)
    return torch.where(x.abs() < 2.0 ** -8, tiny, x).contiguous()


@functools.lru_cache(maxsize=None)
def _packed(shape, bits, scheme, seed=7):
    """(PackedTensor of a random tensor, its de-quantization) - computed once, never modified."""
    from admmq import quantize_packed
    p = quantize_packed([_randn(shape, seed + 131 * bits + shape[0], 0.3)], bits, scheme)[0]
    return p, p.dequantize()


def _gemm(p, trans, x, layout, bias=None, out_dtype=None):
    from admmq.packed import _meta_words, _weight_dims, packed_gemm
    M, K = _weight_dims(p, trans)
    return packed_gemm(p.codes, _meta_words(p), trans, M, K, x, layout, bias, None, out_dtype)


def _need(p, trans, N, nb):
    from admmq import _lib
    from admmq.packed import _meta_words, _weight_dims
    M, K = _weight_dims(p, trans)
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    return _lib.load().admmq_packed_hgemm_workspace_size(ctypes.byref(meta), M, K, N, nb)


def _raw(p, trans, x, layout, N, nb, bias, y, codes=None, ws=None, ws_bytes=None):
    """admmq_packed_hgemm through ctypes on caller-owned buffers (the dtypes are the tensors')."""
    from admmq import _lib
    from admmq.packed import _meta_words, _weight_dims
    lib = _lib.load()
    M, K = _weight_dims(p, trans)
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    if ws is None:
        ws = torch.empty(max(_need(p, trans, N, nb), 256), dtype=torch.uint8, device=DEV)
        ws_bytes = ws.numel()
    c = p.codes if codes is None else codes
    rc = lib.admmq_packed_hgemm(_lib.ptr(c), ctypes.byref(meta), 1 if trans else 0, M, K, _lib.ptr(x), DT[x.dtype], layout,
                                N, nb, _lib.ptr(bias), _lib.ptr(y), DT[y.dtype], _lib.ptr(ws), ws_bytes,
                                _lib.stream_handle(DEV))
    assert rc == 0, lib.admmq_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------- 1. decode exactness
@pytest.mark.parametrize("bits,scheme", [(b, s) for b in range(1, 9) for s in SCHEMES if not (s == MINMAX and b == 1)])
def test_identity_activations_give_the_decoded_weight(bits, scheme):
    """X = I: the sum is one product of the exact integer operand by 1.0 plus exact zeros, the epilogue is
    dequant_code's operations in its order (tensor_minmax: S_x = 1 exactly), so the float32 result is
    torch.equal to dequantize_packed and the half result to its conversion - both orientations, both
    layouts, both dtypes."""
    for shape in [(64, 134), (134, 9), (33, 65), (1, 7)]:
        p, D = _packed(shape, bits, scheme)
        for trans in (False, True):
            W = D.T if trans else D                      # [M, K]
            K = W.shape[1]
            for dtype in DTYPES:
                eye = torch.eye(K, device=DEV, dtype=dtype)
                what = (shape, trans, dtype)
                assert torch.equal(_gemm(p, trans, eye[None], 0, None, torch.float32)[0], W), (what, "nchw")
                assert torch.equal(_gemm(p, trans, eye, 1, None, torch.float32), W.T), (what, "linear")
                y = _gemm(p, trans, eye[None], 0)
                assert y.dtype == dtype and torch.equal(y[0], W.to(dtype)), (what, "nchw half")
                y = _gemm(p, trans, eye, 1)
                assert y.dtype == dtype and torch.equal(y, W.T.to(dtype)), (what, "linear half")


# ------------------------------------------------------------------------- 2. the bound
RATIOS = []


def _check_bound(y, p, Wd, x_kn, bias, what):
    """|y - y64| <= (K + 4) 2^-23 mag elementwise in float64; x_kn: [nb, K, N] (half values). mag = |D||x| + |bias|
    for the scale schemes, (|D - mn| + |mn|)|x| + |bias| for tensor_minmax. Derived: at most 3 roundings in the
    decode / epilogue identity, a K-term float32 sum in any order at one full ulp per add, the bias add."""
    K = Wd.shape[1]
    W64, X64 = Wd.double().cpu(), x_kn.double().cpu()
    yd = W64 @ X64
    if p.qscheme == MINMAX:
        mag = ((W64 - p.mn).abs() + abs(p.mn)) @ X64.abs()
    else:
        mag = W64.abs() @ X64.abs()
    if bias is not None:
        yd = yd + bias.double().cpu()[None, :, None]
        mag = mag + bias.double().cpu().abs()[None, :, None]
    err = (y.double().cpu() - yd).abs()
    bound = (K + 4) * ULP * mag
    ratio = float((err / bound.clamp_min(1e-300)).max())
    RATIOS.append(ratio)
    print(f"{what}: max |err| / bound = {ratio:.4f} (largest so far {max(RATIOS):.4f})")
    assert y.dtype == torch.float32 and torch.isfinite(y).all()
    assert bool((err <= bound).all()), f"{what}: max |err| / bound = {ratio}"


BITS_SCHEMES = [(3, AFF), (4, MSE), (8, MINMAX), (4, SYM)]
NCHW = [(64, 134, 49, 3), (134, 64, 1, 1), (33, 65, 70, 1), (512, 1141, 4, 1), (1141, 512, 49, 1)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,N,nb", NCHW)
def test_nchw_bound_against_float64_and_conversion(M, K, N, nb, dtype):
    """(512, 1141, 4, 1) is the weight-streaming regime (pieces as separate workgroups + the ordered reduction).
    With bias also test 3: the half result is the float32 result converted once."""
    x = _hx((nb, K, N), 11, dtype)
    bias = _randn((M,), 12)
    for bits, scheme in BITS_SCHEMES:
        for trans in (False, True):
            p, D = _packed((K, M) if trans else (M, K), bits, scheme)
            Wd = D.T if trans else D
            for b in (None, bias):
                y = _gemm(p, trans, x, 0, b, torch.float32)
                assert tuple(y.shape) == (nb, M, N)
                _check_bound(y, p, Wd, x, b, f"nchw {(M, K, N, nb)} {dtype} bits {bits} trans {trans} bias {b is not None}")
            yh = _gemm(p, trans, x, 0, bias)
            assert yh.dtype == dtype and torch.equal(yh, y.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tokens", [1, 5, 70])
@pytest.mark.parametrize("shape", [(64, 134), (134, 64)])
def test_linear_bound_against_float64_and_conversion(shape, tokens, dtype):
    for bits, scheme in BITS_SCHEMES:
        p, D = _packed(shape, bits, scheme)
        for trans in (False, True):
            Wd = D.T if trans else D
            M, K = Wd.shape
            x = _hx((tokens, K), 13, dtype)
            bias = _randn((M,), 14)
            for b in (None, bias):
                y = _gemm(p, trans, x, 1, b, torch.float32)
                assert tuple(y.shape) == (tokens, M)
                _check_bound(y.T[None], p, Wd, x.T[None], b,
                             f"linear {shape} tokens {tokens} {dtype} bits {bits} trans {trans} bias {b is not None}")
            yh = _gemm(p, trans, x, 1, bias)
            assert yh.dtype == dtype and torch.equal(yh, y.to(dtype))
            # a bias of x's dtype is read as float32, exactly
            assert torch.equal(_gemm(p, trans, x, 1, bias.to(dtype)), _gemm(p, trans, x, 1, bias.to(dtype).float()))


# ------------------------------------------------------------ 4. determinism and regimes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,N", [(64, 134, 49), (512, 1141, 4), (33, 65, 70)])
def test_calls_repeat_and_images_do_not_depend_on_the_batch(M, K, N, dtype):
    for scheme in (MSE, MINMAX):
        for trans in (False, True):
            p, _ = _packed((K, M) if trans else (M, K), 4, scheme)
            x = _hx((3, K, N), 17, dtype)
            bias = _randn((M,), 18)
            y1 = _gemm(p, trans, x, 0, bias, torch.float32)
            assert torch.equal(y1, _gemm(p, trans, x, 0, bias, torch.float32))
            for b in range(3):
                yb = _gemm(p, trans, x[b:b + 1].contiguous(), 0, bias, torch.float32)
                assert torch.equal(yb[0], y1[b]), (scheme, trans, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", [MSE, MINMAX])
def test_serial_and_parallel_regimes_give_the_same_bits(scheme, dtype):
    """(64, 134) on 16384 tokens: 256 column tiles, the serial regime with 3 pieces; one row alone: one tile, the
    pieces as separate workgroups and the ordered reduction (tensor_minmax: the column sums of x too)."""
    from admmq import _lib
    p, _ = _packed((64, 134), 4, scheme)
    assert _need(p, False, 16384, 1) == 0 and _need(p, False, 1, 1) > 0
    assert _lib.load().admmq_packed_gemm_workspace_size(64, 134, 1, 1) == 3 * 64 * 4
    assert _need(p, False, 1, 1) == 3 * 64 * 4 + (3 * 4 if scheme == MINMAX else 0)
    x = _hx((16384, 134), 19, dtype)
    bias = _randn((64,), 20)
    big = _gemm(p, False, x, 1, bias, torch.float32)
    one = _gemm(p, False, x[5:6].contiguous(), 1, bias, torch.float32)
    assert torch.equal(one[0], big[5])
    assert torch.equal(_gemm(p, False, x[5:6].contiguous(), 1, bias)[0], _gemm(p, False, x, 1, bias)[5])


# ----------------------------------------------------------------------------- 5. bounds of access
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,bits,N,nb", [((33, 65), 3, 70, 1), ((134, 9), 5, 3, 2), ((510, 1141), 3, 4, 1)])
def test_nothing_outside_the_stream_the_output_or_the_workspace_is_touched(shape, bits, N, nb, dtype):
    from admmq.packed import packed_bytes
    nbytes = packed_bytes(shape[0] * shape[1], bits)
    canary = -12288.0   # (exact in bf16 and fp16)
    for scheme in (SYM, MINMAX):
        p, _ = _packed(shape, bits, scheme)
        assert nbytes % 4 != 0 and p.codes.numel() == nbytes
        for trans in (False, True):
            M, K = (shape[1], shape[0]) if trans else shape
            x = _hx((nb, K, N), 20, dtype)
            bias = _randn((M,), 21)
            total = nb * M * N
            ref = _gemm(p, trans, x, 0, bias)
            outs = []
            for fill in (0x00, 0xFF):
                cbuf = torch.full((64 + nbytes + 512,), fill, dtype=torch.uint8, device=DEV)
                cview = cbuf[64:64 + nbytes]
                assert cview.data_ptr() % 16 == 0
                cview.copy_(p.codes)
                ybuf = torch.full((total + 128,), canary, device=DEV, dtype=dtype)
                need = _need(p, trans, N, nb)
                ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
                _raw(p, trans, x, 0, N, nb, bias, ybuf[64:64 + total], codes=cview, ws=ws, ws_bytes=need + 256)
                assert bool((ybuf[:64] == canary).all()) and bool((ybuf[64 + total:] == canary).all())
                assert bool((ws[need:] == 0xA5).all())
                assert bool((cbuf[:64] == fill).all()) and bool((cbuf[64 + nbytes:] == fill).all())
                outs.append(ybuf[64:64 + total].clone())
            assert torch.equal(outs[0], outs[1])
            assert torch.equal(outs[0].view(ref.shape), ref)   # ... and the ctypes route equals the op's


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,N,nb,layout", [(64, 134, 49, 3, 0), (512, 1141, 4, 1, 0), (134, 64, 70, 1, 1),
                                             (64, 136, 70, 1, 1), (512, 1141, 5, 1, 1)])
def test_element_aligned_activations_outputs_and_bias(M, K, N, nb, layout, dtype):
    """x, y and bias one element past a 16-byte boundary: the bits of the aligned call (K = 136: the aligned
    call loads 16 bytes at a time, this one element by element)."""
    for trans in (False, True):
        p, _ = _packed((K, M) if trans else (M, K), 4, MSE)
        x = _hx((nb, K, N), 15, dtype) if layout == 0 else _hx((N, K), 15, dtype)
        bias = _randn((M,), 16)
        for ydt in (dtype, torch.float32):
            y_al = _gemm(p, trans, x, layout, bias, ydt)
            xo = torch.empty(x.numel() + 8, device=DEV, dtype=dtype)
            xo = xo[(16 - xo.data_ptr() % 16) % 16 // 2 + 1:][:x.numel()]
            bo = torch.empty(M + 1, device=DEV)[1:]
            yo = torch.empty(y_al.numel() + 1, device=DEV, dtype=ydt)[1:]
            assert xo.data_ptr() % 16 == 2 and bo.data_ptr() % 16 == 4 and yo.data_ptr() % 16 == yo.element_size()
            xo.copy_(x.reshape(-1))
            bo.copy_(bias)
            _raw(p, trans, xo, layout, N, nb, bo, yo)
            assert torch.equal(yo.view(y_al.shape), y_al), (trans, ydt)


# ----------------------------------------------------------------------------- 6. layers
def _factors(shapes, seed):
    from admmq import quantize_packed
    fl = [_randn(s, seed + i, 0.3) for i, s in enumerate(shapes)]
    return quantize_packed(fl, 4, MSE)


def _stage_check(y, W64, x_kn, bias, dtype, what):
    """One packed stage with a half output against float64 on the stage's own (half) input:
    |y - y64| <= B + u (|y64| + B), B the float32 bound of test 2, u the unit roundoff of the conversion."""
    K = W64.shape[1]
    X64 = x_kn.double().cpu()
    yd = W64 @ X64
    mag = W64.abs() @ X64.abs()
    if bias is not None:
        yd = yd + bias.double().cpu()[None, :, None]
        mag = mag + bias.double().cpu().abs()[None, :, None]
    B = (K + 4) * ULP * mag
    bound = B + UNIT[dtype] * (yd.abs() + B)
    err = (y.double().cpu() - yd).abs()
    print(f"{what}: max |err| / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f}")
    assert y.dtype == dtype and bool((err <= bound).all()), what


def _rel_fro(y, y64):
    y64 = y64.detach()
    return float((y.detach().double().cpu() - y64).norm() / y64.norm())


@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_linear_and_conv1x1_modules_on_half_inputs(dtype):
    """Before .half() (float32 bias) and after (half bias, read exactly): the stage bound, and the float64-layer
    distance of the float tests (1e-5) plus one conversion's unit roundoff."""
    from admmq import export
    p, D = _packed((70, 134), 4, MSE)
    bias = _randn((70,), 41)
    cast = (lambda m: m.half()) if dtype == torch.float16 else (lambda m: m.bfloat16())
    x = _hx((3, 5, 134), 42, dtype)
    xc = _hx((2, 134, 7, 5), 43, dtype)
    for half_module in (False, True):
        lin, conv = export.PackedLinear(p, bias), export.PackedConv1x1(p, bias)
        if half_module:
            lin, conv = cast(lin), cast(conv)
            assert lin.bias.dtype == dtype and lin.codes.dtype == torch.uint8 and torch.equal(lin.codes, p.codes)
        b = lin.bias.detach()
        y = lin(x)
        assert tuple(y.shape) == (3, 5, 70)
        _stage_check(y.reshape(15, 70).T[None], D.double().cpu(), x.reshape(15, 134).T[None], b, dtype,
                     f"PackedLinear {dtype} half module {half_module}")
        y64 = x.double().cpu() @ D.double().cpu().T + b.double().cpu()
        assert _rel_fro(y, y64) <= 1e-5 + UNIT[dtype]
        yc = conv(xc)
        assert tuple(yc.shape) == (2, 70, 7, 5)
        _stage_check(yc.reshape(2, 70, 35), D.double().cpu(), xc.reshape(2, 134, 35), b, dtype,
                     f"PackedConv1x1 {dtype} half module {half_module}")
        with pytest.raises(TypeError, match="float32 tensors required"):
            lin(x.double())
    lin = export.PackedLinear(p, bias)
    lin.set_activation_quant(4, -1.0, 1.0)
    with pytest.raises(ValueError, match="act="):
        lin(x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unfused_cp2conv_layer_on_half_inputs(dtype):
    """build_cp2conv_layer's two packed 1x1 stages on a half input: each stage inside its bound on its own input,
    the layer the composition of its stages, and the float64-layer distance of the float test (1e-5) plus one
    unit roundoff per stage output."""
    from admmq import export
    cout, cin, R = 128, 64, 40
    pf = _factors([(cout, R), (cin, R)], 30)
    deq = [q.dequantize() for q in pf]
    bias = _randn((cout,), 31)
    x = _hx((2, cin, 8, 8), 32, dtype)
    ref = export.build_cp2conv_layer(R, [d.cpu() for d in deq], bias.cpu(), cin, cout, 0, 2).double()
    y64 = ref(x.double().cpu())
    for half_module in (False, True):
        seq = export.build_cp2conv_layer(R, pf, bias, cin, cout, 0, 2)
        if half_module:
            seq = seq.half() if dtype == torch.float16 else seq.bfloat16()
        y = seq(x)
        assert y.dtype == dtype and y.shape == y64.shape
        xs = x[:, :, ::2, ::2].contiguous()
        h = seq.conv1(x)
        _stage_check(h.reshape(2, R, 16), deq[1].T.double().cpu(), xs.reshape(2, cin, 16), None, dtype, "cp2conv stage 1")
        _stage_check(y.reshape(2, cout, 16), deq[0].double().cpu(), h.reshape(2, R, 16), seq.conv2.bias.detach(), dtype,
                     "cp2conv stage 2")
        assert torch.equal(seq.conv2(h), y)
        rel = _rel_fro(y, y64)
        print(f"build_cp2conv_layer {dtype} half module {half_module}: rel Frobenius {rel:.3e}")
        assert rel <= 1e-5 + 2 * UNIT[dtype]


def test_lowrank_linear_on_bf16_is_the_documented_composition():
    """(K + r + 6) 2^-23 (|D||x| + |L|(|Rt||x|) + |bias|) with float32 out: DESIGN.md 2.28's bound with a full ulp
    per operation; the module's bf16 result is that result converted once."""
    from admmq import PackedLowRank, export, packed_lowrank_linear
    M, K, r = 134, 200, 24
    p, D = _packed((M, K), 4, MSE)
    L, Rt, bias = _randn((M, r), 50, 0.1), _randn((r, K), 51, 0.1), _randn((M,), 52)
    x = _hx((37, K), 53, torch.bfloat16)
    plr = PackedLowRank(p, L, Rt)
    y = packed_lowrank_linear(x, plr, bias, out_dtype=torch.float32)
    assert y.dtype == torch.float32 and tuple(y.shape) == (37, M)
    X, D64, L64, R64 = x.double().cpu(), D.double().cpu(), L.double().cpu(), Rt.double().cpu()
    y64 = X @ D64.T + (X @ R64.T) @ L64.T + bias.double().cpu()
    mag = X.abs() @ D64.abs().T + (X.abs() @ R64.abs().T) @ L64.abs().T + bias.double().cpu().abs()
    err = (y.double().cpu() - y64).abs()
    bound = (K + r + 6) * ULP * mag
    print(f"lowrank bf16: max |err| / bound = {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())
    mod = export.PackedLowRankLinear(plr, bias)
    assert torch.equal(mod(x), y.to(torch.bfloat16))
    assert torch.equal(packed_lowrank_linear(x, plr, bias), y.to(torch.bfloat16))
    half = export.PackedLowRankLinear(plr, bias).bfloat16()
    yh = half(x)
    assert yh.dtype == torch.bfloat16 and half.L.dtype == torch.bfloat16 and _rel_fro(yh, y64) <= 3 * UNIT[torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES)
def test_ops_route_and_ctypes_route_give_the_same_bits(dtype, monkeypatch):
    from admmq import _lib
    cases = [((64, 134), 4, MSE, 0), ((512, 1141), 8, MINMAX, 0), ((134, 64), 3, AFF, 1), ((512, 1141), 4, SYM, 1)]
    for shape, bits, scheme, layout in cases:
        p, _ = _packed(shape, bits, scheme)
        x = _hx((2, shape[1], 5), 60, dtype) if layout == 0 else _hx((3, shape[1]), 60, dtype)
        bias = _randn((shape[0],), 61)
        for od in (None, torch.float32):
            assert _lib.use_ops()
            a = _gemm(p, False, x, layout, bias, od)
            with monkeypatch.context() as mp:
                mp.setattr(_lib, "use_ops", lambda: False)
                b = _gemm(p, False, x, layout, bias, od)
            assert a.dtype == b.dtype and torch.equal(a, b), (shape, scheme, layout, od)


def test_inference_only_and_compile_opaque():
    from admmq import _lib, packed_linear
    from admmq.packed import _meta_words
    p, _ = _packed((64, 134), 4, MSE)
    x = _hx((3, 134), 70, torch.bfloat16).requires_grad_()
    with pytest.raises(RuntimeError, match="inference only"):
        packed_linear(x, p)
    with pytest.raises(RuntimeError, match="inference only"):
        _lib.ops().packed_hgemm(p.codes, _meta_words(p), False, 64, 134, x, 1, None, False)
    with torch.no_grad():
        y = packed_linear(x, p)
    assert not y.requires_grad and torch.equal(y, packed_linear(x.detach(), p))
    from admmq.packed import _opaque_packed_hgemm, _packed_hgemm
    assert _opaque_packed_hgemm is not _packed_hgemm   # the torch.compile route is a disabled (opaque) call
