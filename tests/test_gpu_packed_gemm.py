"""Packed-weight GEMM on the MI355X: k_packed_gemm decodes exactly
dequantize_packed's weight (identity activations: bit-exact), its sums meet the forward
bound of a length-K float32 FMA sum in any order against float64, the result does not
depend on the call or the batch, nothing outside the stream / the output / the workspace
is touched, and the export builders run the reference's layer layouts on PackedTensor
factors without a float32 copy of a large factor."""
import ctypes
import functools

import pytest
import torch
from torch import nn

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE, MINMAX, SYM, AFF = "tensor_mseminmax_symmetric", "tensor_minmax", "tensor_symmetric", "tensor_affine"
SCHEMES = [MSE, MINMAX, SYM, AFF]
DEV = torch.device("cuda:0")
U = 2.0 ** -24


def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


@functools.lru_cache(maxsize=None)
def _packed(shape, bits, scheme, seed=7):
    """(PackedTensor of a random tensor, its de-quantization) - computed once, never modified."""
    from admmq import quantize_packed
    p = quantize_packed([_randn(shape, seed + 131 * bits + shape[0], 0.3)], bits, scheme)[0]
    return p, p.dequantize()


def _gemm(p, trans, x, layout, bias=None):
    from admmq.packed import _meta_words, _weight_dims, packed_gemm
    M, K = _weight_dims(p, trans)
    return packed_gemm(p.codes, _meta_words(p), trans, M, K, x, layout, bias)


def _raw(p, trans, x, layout, N, nb, bias, y, codes=None, ws=None, ws_bytes=None):
    """admmq_packed_gemm through ctypes on caller-owned buffers; returns the workspace used."""
    from admmq import _lib
    from admmq.packed import _meta_words, _weight_dims
    lib = _lib.load()
    M, K = _weight_dims(p, trans)
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    need = lib.admmq_packed_gemm_workspace_size(M, K, N, nb)
    if ws is None:
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
        ws_bytes = ws.numel()
    c = p.codes if codes is None else codes
    rc = lib.admmq_packed_gemm(_lib.ptr(c), ctypes.byref(meta), 1 if trans else 0, M, K, _lib.ptr(x), layout, N, nb,
                               _lib.ptr(bias), _lib.ptr(y), _lib.ptr(ws), ws_bytes, _lib.stream_handle(DEV))
    assert rc == 0, lib.admmq_last_error()
    torch.cuda.synchronize()
    return need


# ------------------------------------------------------------------- decode exactness
@pytest.mark.parametrize("bits,scheme", [(b, s) for b in range(1, 9) for s in SCHEMES if not (s == MINMAX and b == 1)])
def test_identity_activations_give_the_decoded_weight(bits, scheme):
    """X = I: every output is one product by 1.0 plus exact zeros, so any summation order
    returns the decoded weight itself - torch.equal to dequantize_packed, both orientations,
    both activation layouts. Shapes: rows starting mid-byte, a stream ending mid-dword, sizes
    on either side of 32 and 64 (tensor_minmax has no 1-bit code)."""
    for shape in [(64, 134), (134, 9), (33, 65), (1, 7)]:
        p, D = _packed(shape, bits, scheme)
        for trans in (False, True):
            W = D.T if trans else D                      # [M, K]
            K = W.shape[1]
            eye = torch.eye(K, device=DEV)
            y = _gemm(p, trans, eye[None], 0)            # [1, M, K]
            assert torch.equal(y[0], W), (shape, trans, "nchw")
            y = _gemm(p, trans, eye, 1)                  # [K tokens, M] = W^T
            assert torch.equal(y, W.T), (shape, trans, "linear")


# ------------------------------------------------------------------------- accuracy
def _check_bound(y, Wd, x_kn, bias, what):
    """|Y - Yd| <= (K + 2) 2^-24 (|Wd| |X| + |bias|) elementwise in float64; x_kn: [nb, K, N]."""
    K = Wd.shape[1]
    W64, X64 = Wd.double().cpu(), x_kn.double().cpu()
    yd = W64 @ X64
    mag = W64.abs() @ X64.abs()
    if bias is not None:
        yd = yd + bias.double().cpu()[None, :, None]
        mag = mag + bias.double().cpu().abs()[None, :, None]
    err = (y.double().cpu() - yd).abs()
    bound = (K + 2) * U * mag
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |err| / bound = {ratio:.4f}")
    assert torch.isfinite(y).all()
    assert bool((err <= bound).all()), f"{what}: max |err| / bound = {ratio}"


BITS_SCHEMES = [(3, AFF), (4, MSE), (8, MINMAX), (4, SYM)]


@pytest.mark.parametrize("M,K,N,nb", [(64, 134, 49, 3), (134, 64, 1, 1), (134, 64, 65, 2), (33, 65, 70, 1),
                                      (512, 1141, 4, 1), (1141, 512, 49, 1)])
def test_nchw_accuracy_against_float64(M, K, N, nb):
    """Both orientations, with and without bias, bits 3 / 4 / 8; (512, 1141, 4, 1) is the
    weight-streaming regime (K pieces as separate workgroups + the ordered reduction)."""
    x = _randn((nb, K, N), 11)
    bias = _randn((M,), 12)
    for bits, scheme in BITS_SCHEMES:
        for trans in (False, True):
            p, D = _packed((K, M) if trans else (M, K), bits, scheme)
            Wd = D.T if trans else D
            for b in (None, bias):
                y = _gemm(p, trans, x, 0, b)
                assert tuple(y.shape) == (nb, M, N)
                _check_bound(y, Wd, x, b, f"nchw {(M, K, N, nb)} bits {bits} trans {trans} bias {b is not None}")


@pytest.mark.parametrize("tokens", [1, 5, 70])
@pytest.mark.parametrize("shape", [(64, 134), (134, 64)])
def test_linear_accuracy_against_float64(shape, tokens):
    for bits, scheme in BITS_SCHEMES:
        p, D = _packed(shape, bits, scheme)
        for trans in (False, True):
            Wd = D.T if trans else D
            M, K = Wd.shape
            x = _randn((tokens, K), 13)
            bias = _randn((M,), 14)
            for b in (None, bias):
                y = _gemm(p, trans, x, 1, b)
                assert tuple(y.shape) == (tokens, M)
                _check_bound(y.T[None], Wd, x.T[None], b,
                             f"linear {shape} tokens {tokens} bits {bits} trans {trans} bias {b is not None}")


@pytest.mark.parametrize("M,K,N,nb,layout", [(64, 134, 49, 3, 0), (512, 1141, 4, 1, 0), (134, 64, 70, 1, 1),
                                             (512, 1141, 5, 1, 1)])
def test_misaligned_activations_outputs_and_bias(M, K, N, nb, layout):
    """x, y and bias 4 bytes past a 16-byte boundary (ctypes route: the test owns the buffers):
    the same bits as the aligned call, inside the float64 bound."""
    for trans in (False, True):
        p, D = _packed((K, M) if trans else (M, K), 4, MSE)
        Wd = D.T if trans else D
        x = _randn((nb, K, N), 15) if layout == 0 else _randn((N, K), 15)
        bias = _randn((M,), 16)
        y_al = _gemm(p, trans, x, layout, bias)
        xo = torch.empty(x.numel() + 1, device=DEV)[1:]
        bo = torch.empty(M + 1, device=DEV)[1:]
        yo = torch.empty(y_al.numel() + 1, device=DEV)[1:]
        assert xo.data_ptr() % 16 == 4 and bo.data_ptr() % 16 == 4 and yo.data_ptr() % 16 == 4
        xo.copy_(x.reshape(-1))
        bo.copy_(bias)
        _raw(p, trans, xo, layout, N, nb, bo, yo)
        y = yo.view(y_al.shape)
        assert torch.equal(y, y_al)
        if layout == 0:
            _check_bound(y, Wd, x, bias, f"misaligned nchw {(M, K, N, nb)} trans {trans}")
        else:
            _check_bound(y.T[None], Wd, x.T[None], bias, f"misaligned linear {(M, K, N)} trans {trans}")


# ------------------------------------------------------------ determinism and batching
@pytest.mark.parametrize("M,K,N", [(64, 134, 49), (512, 1141, 4), (1141, 512, 49), (33, 65, 70)])
def test_calls_repeat_and_images_do_not_depend_on_the_batch(M, K, N):
    for trans in (False, True):
        p, _ = _packed((K, M) if trans else (M, K), 4, MSE)
        x = _randn((3, K, N), 17)
        bias = _randn((M,), 18)
        y1 = _gemm(p, trans, x, 0, bias)
        y2 = _gemm(p, trans, x, 0, bias)
        assert torch.equal(y1, y2)
        for b in range(3):
            yb = _gemm(p, trans, x[b:b + 1].contiguous(), 0, bias)
            assert torch.equal(yb[0], y1[b]), (trans, b)


def test_linear_calls_repeat():
    p, _ = _packed((512, 1141), 4, MSE)
    x = _randn((4, 1141), 19)
    assert torch.equal(_gemm(p, False, x, 1), _gemm(p, False, x, 1))
    # a row of a larger call equals the call on that row alone (the K order is a function of K)
    assert torch.equal(_gemm(p, False, x[2:3].contiguous(), 1)[0], _gemm(p, False, x, 1)[2])


@pytest.mark.parametrize("scheme", [MSE, MINMAX])
@pytest.mark.parametrize("trans", [False, True])
def test_ops_route_and_ctypes_route_give_the_same_bits(scheme, trans, monkeypatch):
    """The plain call (no ``act``) through torch.ops.admmq and, with ``use_ops`` off, through ctypes (DESIGN.md
    2.30): a 3-bit 70 x 100 weight, whose code runs straddle dwords, on a linear and a channel-first ``x``."""
    from admmq import _lib, packed_linear
    p, _ = _packed((100, 70) if trans else (70, 100), 3, scheme)
    bias = _randn((70,), 38)
    calls = [lambda: packed_linear(_randn((3, 100), 36), p, None, trans),
             lambda: packed_linear(_randn((3, 100), 36), p, bias, trans),
             lambda: _gemm(p, trans, _randn((2, 100, 5), 37), 0),
             lambda: _gemm(p, trans, _randn((2, 100, 5), 37), 0, bias)]
    for i, call in enumerate(calls):
        assert _lib.use_ops()
        a = call()
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "use_ops", lambda: False)
            b = call()
        assert tuple(a.shape) == ((3, 70), (3, 70), (2, 70, 5), (2, 70, 5))[i] and torch.equal(a, b), i


# ----------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("shape,bits,N,nb", [((33, 65), 3, 70, 1), ((134, 9), 5, 3, 2), ((510, 1141), 3, 4, 1)])
def test_nothing_outside_the_stream_the_output_or_the_workspace_is_touched(shape, bits, N, nb):
    from admmq import _lib
    from admmq.packed import packed_bytes
    p, _ = _packed(shape, bits, SYM)
    nbytes = packed_bytes(shape[0] * shape[1], bits)
    assert nbytes % 4 != 0 and p.codes.numel() == nbytes
    for trans in (False, True):
        M, K = (shape[1], shape[0]) if trans else shape
        x = _randn((nb, K, N), 20)
        bias = _randn((M,), 21)
        total = nb * M * N
        ref = _gemm(p, trans, x, 0, bias)
        outs = []
        for fill in (0x00, 0xFF):
            cbuf = torch.full((64 + nbytes + 512,), fill, dtype=torch.uint8, device=DEV)
            cview = cbuf[64:64 + nbytes]
            assert cview.data_ptr() % 16 == 0
            cview.copy_(p.codes)
            ybuf = torch.full((total + 128,), -12345.5, device=DEV)
            need = _lib.load().admmq_packed_gemm_workspace_size(M, K, N, nb)
            ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
            _raw(p, trans, x, 0, N, nb, bias, ybuf[64:64 + total], codes=cview, ws=ws, ws_bytes=need + 256)
            assert bool((ybuf[:64] == -12345.5).all()) and bool((ybuf[64 + total:] == -12345.5).all())
            assert bool((ws[need:] == 0xA5).all())
            assert bool((cbuf[:64] == fill).all()) and bool((cbuf[64 + nbytes:] == fill).all())
            outs.append(ybuf[64:64 + total].clone())
        assert torch.equal(outs[0], outs[1])
        assert torch.equal(outs[0].view(ref.shape), ref)   # ... and the ctypes route equals the op's


# ----------------------------------------------------------------------------- layers
def _rel_fro(y, y64):
    y64 = y64.detach()
    return float((y.detach().double().cpu() - y64).norm() / y64.norm())


def _factors(shapes, seed):
    from admmq import quantize_packed
    fl = [_randn(s, seed + i, 0.3) for i, s in enumerate(shapes)]
    return quantize_packed(fl, 4, MSE)


def _float64_layer(build, deq):
    return build([d.cpu() for d in deq]).double()


@pytest.mark.parametrize("cout,cin,k,R,stride", [(64, 64, 3, 134, 1), (128, 64, 1, 40, 2)])
def test_factorized_conv_on_packed_factors(cout, cin, k, R, stride, tmp_path):
    from admmq import export
    conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=True).to(DEV)
    shapes = [(cout, R), (cin, R)] + ([(k * k, R)] if k > 1 else [])
    pf = _factors(shapes, 30)
    seq = export.factorized_conv(conv, R, pf)
    names = [n for n, _ in seq.named_children()]
    first, last = seq.conv1, (seq.conv3 if k > 1 else seq.conv2)
    if k > 1:
        assert names == ["conv1", "conv2", "conv3"] and type(seq.conv2) is nn.Conv2d and seq.conv2.groups == R
        assert tuple(seq.conv2.weight.shape) == (R, 1, k, k)
    else:
        assert names == ["conv1", "conv2"]
    for m, (M, K, tr) in ((first, (R, cin, True)), (last, (cout, R, False))):
        assert type(m) is export.PackedConv1x1 and m.transpose is tr and (m.out_features, m.in_features) == (M, K)
        assert not hasattr(m, "weight")
        for t in list(m.parameters()) + list(m.buffers()):
            assert not (t.dtype == torch.float32 and t.numel() >= M * K)
        assert m.codes.dtype == torch.uint8 and m.codes.numel() == M * K // 2
    x = _randn((2, cin, 8, 8), 31)
    y = seq(x)
    deq = [p.dequantize() for p in pf]
    ref = _float64_layer(lambda f: export.factorized_conv(conv.cpu(), R, f), deq)
    conv.to(DEV)
    y64 = ref(x.double().cpu())
    assert y.shape == y64.shape
    rel = _rel_fro(y, y64)
    print(f"factorized_conv {(cout, cin, k, R, stride)}: rel Frobenius {rel:.3e}")
    assert rel <= 1e-5
    # state_dict -> torch.save -> a fresh module (other codes) -> load_state_dict: the same bits
    path = str(tmp_path / "layer.pt")
    torch.save(seq.state_dict(), path)
    fresh = export.factorized_conv(conv, R, _factors(shapes, 77))
    assert not torch.equal(fresh(x), y)
    fresh.load_state_dict(torch.load(path, map_location=DEV, weights_only=True))
    assert torch.equal(fresh(x), y)
    assert torch.equal(last.dequantize(), deq[0]) and torch.equal(first.dequantize(), deq[1].T)


def test_cpfc_layer_on_packed_factors(tmp_path):
    from admmq import export
    fout, fin, R = 70, 64, 24
    pf = _factors([(fout, R), (fin, R)], 40)      # [B, A]
    bias = _randn((fout,), 41)
    seq = export.build_cpfc_layer(R, pf, bias, fin, fout)
    assert [n for n, _ in seq.named_children()] == ["fc1", "fc2"]
    assert type(seq.fc1) is export.PackedLinear and seq.fc1.transpose and type(seq.fc2) is export.PackedLinear
    for m, (M, K) in ((seq.fc1, (R, fin)), (seq.fc2, (fout, R))):
        assert (m.out_features, m.in_features) == (M, K) and not hasattr(m, "weight")
        for t in list(m.parameters()) + list(m.buffers()):
            assert not (t.dtype == torch.float32 and t.numel() >= M * K)
    x = _randn((3, 5, fin), 42)
    y = seq(x)
    deq = [p.dequantize() for p in pf]
    ref = _float64_layer(lambda f: export.build_cpfc_layer(R, f, bias.cpu(), fin, fout), deq)
    y64 = ref(x.double().cpu())
    rel = _rel_fro(y, y64)
    print(f"build_cpfc_layer: rel Frobenius {rel:.3e}")
    assert y.shape == y64.shape and rel <= 1e-5
    path = str(tmp_path / "fc.pt")
    torch.save(seq.state_dict(), path)
    fresh = export.build_cpfc_layer(R, _factors([(fout, R), (fin, R)], 78), torch.zeros(fout, device=DEV), fin, fout)
    fresh.load_state_dict(torch.load(path, map_location=DEV, weights_only=True))
    assert torch.equal(fresh(x), y)


def test_inference_only():
    from admmq import export, packed_linear
    p, _ = _packed((64, 134), 4, MSE)
    x = _randn((3, 134), 50).requires_grad_()
    with pytest.raises(RuntimeError, match="inference only"):
        packed_linear(x, p)
    with pytest.raises(RuntimeError, match="inference only"):
        export.PackedLinear(p)(x)
    from admmq import _lib
    from admmq.packed import _meta_words
    with pytest.raises(RuntimeError, match="inference only"):
        _lib.ops().packed_gemm(p.codes, _meta_words(p), False, 64, 134, x, 1, None)
    with torch.no_grad():
        y = packed_linear(x, p)
    assert not y.requires_grad and torch.equal(y, packed_linear(x.detach(), p))


def test_factorize_cli_packed_files_build_the_packed_layer(tmp_path):
    """python -m admmq.factorize --save-packed -> load_packed_factors -> factorized_conv -> forward."""
    from admmq import export, factorize, synthetic
    model, layer = "resnet18", "layer1.0.conv1"
    argv = ["--model-name", model, "--method", "admm", "--layer", layer, "--reduction-rate", "2.0", "--bits", "4",
            "--seed", "42", "--qscheme", MSE, "--max_iter_als", "2", "--max_iter_admm", "10",
            "--outdir-root", str(tmp_path), "--save-packed"]
    factorize.main(argv)
    idx, spec = synthetic.find_layer(model, layer)
    cout, cin = spec.shape[0], spec.shape[1]
    R = spec.rank()
    prefix = export.factor_prefix(str(tmp_path), 4, MSE, "admm", 42, layer, "random", R)
    pf = export.load_packed_factors(prefix, 3, DEV)
    assert [tuple(p.shape) for p in pf] == [(cout, R), (cin, R), (9, R)] and all(p.bits == 4 for p in pf)
    conv = nn.Conv2d(cin, cout, 3, padding=1, bias=False).to(DEV)
    seq = export.factorized_conv(conv, R, pf)
    assert type(seq.conv1) is export.PackedConv1x1 and type(seq.conv3) is export.PackedConv1x1
    x = _randn((2, cin, 8, 8), 60)
    y = seq(x)
    deq = export.load_factors(prefix, 3, DEV, packed=True)
    ref = export.factorized_conv(conv.cpu(), R, [d.cpu() for d in deq]).double()
    y64 = ref(x.double().cpu())
    rel = _rel_fro(y, y64)
    print(f"factorize --save-packed -> packed layer: rel Frobenius {rel:.3e}")
    assert rel <= 1e-5


# ----------------------------------------------------------------------------- memory
def test_the_float32_weight_is_never_materialised():
    from admmq import export
    from admmq.packed import packed_bytes
    M, K = 512, 1141
    p, _ = _packed((M, K), 4, MSE)
    lin = export.PackedLinear(p)
    resident = sum(b.numel() * b.element_size() for b in lin.buffers()) + \
        sum(q.numel() * q.element_size() for q in lin.parameters())
    assert packed_bytes(M * K, 4) <= resident <= packed_bytes(M * K, 4) + 64
    x = _randn((4, K), 70)
    lin(x)                                   # (libraries loaded, allocator warm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    y = lin(x)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - before
    print(f"PackedLinear {(M, K)} x 4 tokens: peak rise {rise} B (fp32 weight {M * K * 4} B)")
    assert tuple(y.shape) == (4, M) and rise < M * K * 4
