"""Packed quant + low-rank GEMM on the MI355X: y = x (D + L Rt)^T (+ bias) from
packed codes and two thin factors. With L = 0 or Rt = 0 the tail adds exact zeros (packed_linear's
values, both regimes); with x = I the down-projection is exact; the result meets the forward bound
of its float32 sums against float64, does not depend on the call or the batch, needs float
alignment only, touches nothing outside y / the workspace / the code stream, and the export layer
keeps codes and factors and never a float32 weight.

Shapes (M, K, r, tokens): the smallest at which each mechanism can fail."""
import ctypes
import functools

import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE, MINMAX, SYM, AFF = "tensor_mseminmax_symmetric", "tensor_minmax", "tensor_symmetric", "tensor_affine"
BITS_SCHEMES = [(3, AFF), (4, MSE), (8, MINMAX), (4, SYM)]   # as test_gpu_packed_gemm.py
DEV = torch.device("cuda:0")
U = 2.0 ** -24

PARALLEL = (512, 1141, 8, 4)      # 18 pieces as separate workgroups + the tail's + the ordered reduce
SERIAL = (1024, 134, 8, 1024)     # 256 tiles: one workgroup runs its three pieces and the tail
SHAPES = [(64, 134, 8, 5),        # three K pieces, a ragged last step
          (33, 65, 1, 70),        # partial row tile, two column tiles, r = 1
          (134, 64, 33, 1),       # r crossing one 32-step, one token
          PARALLEL, SERIAL]


def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


@functools.lru_cache(maxsize=None)
def _lowrank(M, K, r, bits=4, scheme=MSE):
    """(PackedLowRank of random parts, the de-quantized W_q) - computed once, never modified."""
    from admmq import PackedLowRank, quantize_packed
    q = quantize_packed([_randn((M, K), 7 + 131 * bits + M, 0.3)], bits, scheme)[0]
    p = PackedLowRank(q=q, L=_randn((M, r), 5 + M + r, 0.5), Rt=_randn((r, K), 6 + K + r, 0.5))
    return p, q.dequantize()


def _regimes(M, K, N, r):
    """(the GEMM's pieces run in parallel, the down-projection's do), read off the workspace queries."""
    from admmq import _lib
    lib = _lib.load()
    kp = max(64, 32 * -(-K // 1024))
    pieces = -(-K // kp)
    main = lib.admmq_packed_gemm_workspace_size(M, K, N, 1)
    t = lib.admmq_packed_lrgemm_workspace_size(M, K, N, r) - (main // pieces * (pieces + 1) if main else 0)
    assert t in (4 * N * r, 4 * N * r * pieces)
    return main > 0, pieces > 1 and t == 4 * N * r * pieces


def test_the_shapes_run_in_the_regimes_they_are_named_for():
    M, K, r, N = PARALLEL
    assert _regimes(M, K, N, r) == (True, True)
    M, K, r, N = SERIAL
    assert _regimes(M, K, N, r) == (False, True)
    # a serial down-projection too: one K piece
    assert _regimes(134, 64, 1, 33) == (False, False)


def _bound_check(y, D, L, Rt, x, bias, what):
    """|y - y64| <= (K + r + 4) 2^-24 (|D||x| + |L|(|Rt||x|) + |bias|) elementwise in float64; y [tokens, M]."""
    K, r = D.shape[1], L.shape[1]
    D64, L64, R64, x64 = D.double().cpu(), L.double().cpu(), Rt.double().cpu(), x.double().cpu()
    y64 = x64 @ D64.T + (x64 @ R64.T) @ L64.T
    mag = x64.abs() @ D64.abs().T + (x64.abs() @ R64.abs().T) @ L64.abs().T
    if bias is not None:
        y64 = y64 + bias.double().cpu()
        mag = mag + bias.double().cpu().abs()
    err = (y.double().cpu() - y64).abs()
    bound = (K + r + 4) * U * mag
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |err| / bound = {ratio:.4f}")
    assert torch.isfinite(y).all()
    assert bool((err <= bound).all()), f"{what}: max |err| / bound = {ratio}"


# ----------------------------------------------------------------- 1. the tail adds exact zeros
@pytest.mark.parametrize("M,K,r,N", SHAPES)
def test_zero_factors_give_packed_linear(M, K, r, N):
    from admmq import PackedLowRank, packed_linear, packed_lowrank_linear
    if (M, K, r, N) == PARALLEL:
        assert _regimes(M, K, N, r)[0]
    if (M, K, r, N) == SERIAL:
        assert not _regimes(M, K, N, r)[0]
    x = _randn((N, K), 11)
    bias = _randn((M,), 12)
    for bits, scheme in BITS_SCHEMES:
        p, _ = _lowrank(M, K, r, bits, scheme)
        for b in (None, bias):
            ref = packed_linear(x, p.q, b)
            y = packed_lowrank_linear(x, PackedLowRank(q=p.q, L=torch.zeros_like(p.L), Rt=p.Rt), b)
            assert torch.equal(y, ref), (bits, scheme, "L = 0", b is not None)
            y = packed_lowrank_linear(x, PackedLowRank(q=p.q, L=p.L, Rt=torch.zeros_like(p.Rt)), b)
            assert torch.equal(y, ref), (bits, scheme, "Rt = 0", b is not None)


# ----------------------------------------------------------------- 2. identity activations
@pytest.mark.parametrize("M,K,r", [(64, 134, 8), (33, 65, 1), (134, 64, 33), (512, 1141, 8)])
def test_identity_activations(M, K, r):
    """x = I: t = Rt exactly (one product by 1.0 plus exact zeros in every piece), the code part is D exactly,
    so y^T = D + L Rt up to the r-term tail, the add of the tail and the roundings of D + q."""
    from admmq import packed_lowrank_linear
    for bits, scheme in BITS_SCHEMES:
        p, D = _lowrank(M, K, r, bits, scheme)
        y = packed_lowrank_linear(torch.eye(K, device=DEV), p)      # [K tokens, M]
        D64, L64, R64 = D.double().cpu(), p.L.double().cpu(), p.Rt.double().cpu()
        err = (y.T.double().cpu() - (D64 + L64 @ R64)).abs()
        bound = (r + 3) * U * (D64.abs() + L64.abs() @ R64.abs())
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f"identity {(M, K, r)} bits {bits} {scheme}: max |err| / bound = {ratio:.4f}")
        assert bool((err <= bound).all()), ratio


# ----------------------------------------------------------------- 3. forward bound
@pytest.mark.parametrize("M,K,r,N", SHAPES)
def test_accuracy_against_float64(M, K, r, N):
    from admmq import packed_lowrank_linear
    x = _randn((N, K), 13)
    bias = _randn((M,), 14)
    for bits, scheme in BITS_SCHEMES:
        p, D = _lowrank(M, K, r, bits, scheme)
        for b in (None, bias):
            y = packed_lowrank_linear(x, p, b)
            assert tuple(y.shape) == (N, M)
            _bound_check(y, D, p.L, p.Rt, x, b, f"{(M, K, r, N)} bits {bits} {scheme} bias {b is not None}")


def test_leading_dimensions_are_tokens():
    from admmq import packed_lowrank_linear
    p, _ = _lowrank(64, 134, 8)
    x = _randn((2, 3, 134), 15)
    y = packed_lowrank_linear(x, p)
    assert tuple(y.shape) == (2, 3, 64)
    assert torch.equal(y.reshape(6, 64), packed_lowrank_linear(x.reshape(6, 134), p))


# ----------------------------------------------------------------- 4. determinism, batching, the ctypes route
def _raw(p, x, N, bias, y, L=None, Rt=None, codes=None, ws=None, ws_bytes=None):
    """admmq_packed_lrgemm through ctypes on caller-owned buffers; returns the workspace size it asked for."""
    from admmq import _lib
    from admmq.packed import _lowrank_dims, _meta_words
    lib = _lib.load()
    M, K, r = _lowrank_dims(p)
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p.q).numpy().tobytes())
    need = lib.admmq_packed_lrgemm_workspace_size(M, K, N, r)
    assert need > 0
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        ws_bytes = need
    rc = lib.admmq_packed_lrgemm(_lib.ptr(p.q.codes if codes is None else codes), ctypes.byref(meta), M, K,
                                 _lib.ptr(p.L if L is None else L), _lib.ptr(p.Rt if Rt is None else Rt), r, _lib.ptr(x), N,
                                 _lib.ptr(bias), _lib.ptr(y), _lib.ptr(ws), ws_bytes, _lib.stream_handle(DEV))
    assert rc == 0, lib.admmq_last_error()
    torch.cuda.synchronize()
    return need


@pytest.mark.parametrize("M,K,r,N", SHAPES)
def test_calls_repeat_rows_stand_alone_and_the_ctypes_route_agrees(M, K, r, N):
    from admmq import packed_lowrank_linear
    p, _ = _lowrank(M, K, r)
    x = _randn((N, K), 17)
    bias = _randn((M,), 18)
    y1 = packed_lowrank_linear(x, p, bias)
    assert torch.equal(y1, packed_lowrank_linear(x, p, bias))
    # a row of a larger call equals the call on that row alone (the order is a function of K and r;
    # the two calls may run in different regimes)
    for row in sorted({0, N // 2, N - 1}):
        assert torch.equal(packed_lowrank_linear(x[row:row + 1].contiguous(), p, bias)[0], y1[row]), row
    y = torch.empty(N, M, device=DEV)
    _raw(p, x, N, bias, y)
    assert torch.equal(y, y1)


def test_ops_route_and_ctypes_route_give_the_same_bits(monkeypatch):
    """packed_lowrank_linear through torch.ops.admmq and, with ``use_ops`` off, through ctypes:
    3-bit codes, 5 rows, r = 3, in two regimes of the down-projection."""
    from admmq import _lib, packed_lowrank_linear
    M, N, r = 70, 5, 3
    assert _regimes(M, 100, N, r) != _regimes(M, 40, N, r)
    for K in (100, 40):
        p, _ = _lowrank(M, K, r, 3)
        x = _randn((N, K), 27)
        for bias in (None, _randn((M,), 28)):
            assert _lib.use_ops()
            a = packed_lowrank_linear(x, p, bias)
            with monkeypatch.context() as mp:
                mp.setattr(_lib, "use_ops", lambda: False)
                b = packed_lowrank_linear(x, p, bias)
            assert torch.equal(a, b), (K, bias is None)


# ----------------------------------------------------------------- 5. alignment and bounds
def _off4(t):
    """A copy of ``t`` that starts 4 bytes past a 16-byte boundary."""
    o = torch.empty(t.numel() + 1, device=DEV)[1:]
    assert o.data_ptr() % 16 == 4
    o.copy_(t.reshape(-1))
    return o


@pytest.mark.parametrize("M,K,r,N", [(64, 134, 8, 5), (134, 64, 33, 1), (512, 1141, 8, 4), (33, 65, 1, 70)])
def test_float_alignment_is_enough(M, K, r, N):
    from admmq import packed_lowrank_linear
    p, D = _lowrank(M, K, r)
    x = _randn((N, K), 19)
    bias = _randn((M,), 20)
    y_al = packed_lowrank_linear(x, p, bias)
    yo = torch.empty(N * M + 1, device=DEV)[1:]
    assert yo.data_ptr() % 16 == 4
    _raw(p, _off4(x), N, _off4(bias), yo, L=_off4(p.L), Rt=_off4(p.Rt))
    assert torch.equal(yo.view(N, M), y_al)
    _bound_check(yo.view(N, M), D, p.L, p.Rt, x, bias, f"misaligned {(M, K, r, N)}")


@pytest.mark.parametrize("M,K,r,N,bits", [(33, 65, 1, 70, 3), (134, 9, 5, 3, 5), (510, 1141, 8, 4, 3), (1025, 134, 8, 1024, 3)])
def test_nothing_outside_the_output_the_workspace_or_the_stream_is_touched(M, K, r, N, bits):
    from admmq import _lib, packed_lowrank_linear
    from admmq.packed import packed_bytes
    p, _ = _lowrank(M, K, r, bits, SYM)
    nbytes = packed_bytes(M * K, bits)
    assert nbytes % 4 != 0 and p.q.codes.numel() == nbytes
    x = _randn((N, K), 21)
    bias = _randn((M,), 22)
    ref = packed_lowrank_linear(x, p, bias)
    total = N * M
    outs = []
    for fill in (0x00, 0xFF):
        cbuf = torch.full((64 + nbytes + 512,), fill, dtype=torch.uint8, device=DEV)
        cview = cbuf[64:64 + nbytes]
        assert cview.data_ptr() % 16 == 0
        cview.copy_(p.q.codes)
        ybuf = torch.full((total + 128,), -12345.5, device=DEV)
        need = _lib.load().admmq_packed_lrgemm_workspace_size(M, K, N, r)
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        _raw(p, x, N, bias, ybuf[64:64 + total], codes=cview, ws=ws, ws_bytes=need + 256)
        assert bool((ybuf[:64] == -12345.5).all()) and bool((ybuf[64 + total:] == -12345.5).all())
        assert bool((ws[need:] == 0xA5).all())
        assert bool((cbuf[:64] == fill).all()) and bool((cbuf[64 + nbytes:] == fill).all())
        outs.append(ybuf[64:64 + total].clone())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0].view(N, M), ref)


# ----------------------------------------------------------------- 6. the layer and its memory
def test_layer_round_trips_through_its_state_dict(tmp_path):
    from admmq import export
    M, K, r = 134, 64, 33
    p, D = _lowrank(M, K, r)
    bias = _randn((M,), 30)
    lin = export.build_qlr_layer(p, bias)
    assert type(lin) is export.PackedLowRankLinear and (lin.in_features, lin.out_features, lin.rank) == (K, M, r)
    x = _randn((3, 5, K), 31)
    y = lin(x)
    _bound_check(y.reshape(15, M), D, p.L, p.Rt, x.reshape(15, K), bias, "layer")
    assert torch.equal(lin.dequantize(), D + p.L @ p.Rt)
    path = str(tmp_path / "qlr.pt")
    torch.save(lin.state_dict(), path)
    other, _ = _lowrank(M, K, r, 4, SYM)
    fresh = export.build_qlr_layer(other, torch.zeros(M, device=DEV))
    assert not torch.equal(fresh(x), y)
    fresh.load_state_dict(torch.load(path, map_location=DEV, weights_only=True))
    assert torch.equal(fresh(x), y)


def test_inference_only():
    from admmq import _lib, export, packed_lowrank_linear
    from admmq.packed import _meta_words
    p, _ = _lowrank(64, 134, 8)
    x = _randn((3, 134), 50).requires_grad_()
    with pytest.raises(RuntimeError, match="inference only"):
        packed_lowrank_linear(x, p)
    with pytest.raises(RuntimeError, match="inference only"):
        export.build_qlr_layer(p)(x)
    with pytest.raises(RuntimeError, match="inference only"):
        _lib.ops().packed_lrgemm(p.q.codes, _meta_words(p.q), 64, 134, p.L, p.Rt, x, None)
    with torch.no_grad():
        y = packed_lowrank_linear(x, p)
    assert not y.requires_grad and torch.equal(y, packed_lowrank_linear(x.detach(), p))


def test_resident_bytes_and_forward_peak():
    """The layer holds the code stream and the two factors and nothing of M K float32 elements; a forward's
    peak memory rise stays below one float32 weight (4 M K bytes)."""
    from admmq import export
    from admmq.packed import packed_bytes
    M, K, r, N = 512, 1141, 8, 4
    p, _ = _lowrank(M, K, r)
    lin = export.build_qlr_layer(p)
    floor = packed_bytes(M * K, 4) + 4 * r * (M + K)
    resident = sum(t.numel() * t.element_size() for t in list(lin.parameters()) + list(lin.buffers()))
    assert floor <= resident <= floor + 64 and p.nbytes == floor
    for t in list(lin.parameters()) + list(lin.buffers()):
        assert not (t.dtype == torch.float32 and t.numel() >= M * K)
    x = _randn((N, K), 60)
    lin(x)   # (the workspace cache and the meta words exist from here on)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    y = lin(x)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - before
    print(f"forward peak rise {rise} bytes, 4 M K = {4 * M * K}")
    assert rise < 4 * M * K and tuple(y.shape) == (N, M)
