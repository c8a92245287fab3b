"""Fused depthwise + 1x1 stage on the MI355X: k_packed_dwgemm returns the bits
of packed_conv1x1 on a Z summed tap by tap in float32 on the CPU, meets the forward bound of
that two-stage sum against float64, forms the stencil exactly (identity-like weight, one-hot
taps), does not depend on the call or the batch, touches nothing outside its output and its
workspace, and the fused export layer equals the unfused packed layer."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE, MINMAX, SYM, AFF = "tensor_mseminmax_symmetric", "tensor_minmax", "tensor_symmetric", "tensor_affine"
BITS_SCHEMES = [(3, AFF), (4, MSE), (8, MINMAX), (4, SYM)]
DEV = torch.device("cuda:0")
U = 2.0 ** -24

# (M, K, (H, W), (kh, kw), (ph, pw), (sh, sw), nb)
GEOMS = [
    (64, 134, (7, 7), (3, 3), (1, 1), (1, 1), 3),       # columns cross image boundaries inside a tile; K tail; 3 pieces
    (33, 65, (8, 8), (3, 3), (1, 1), (2, 2), 2),
    (64, 134, (7, 7), (3, 3), (1, 1), (2, 2), 2),       # odd H with stride 2
    (40, 70, (5, 9), (1, 3), (0, 1), (1, 2), 1),
    (64, 134, (9, 9), (5, 5), (2, 2), (1, 1), 1),
    (128, 1141, (4, 4), (3, 3), (1, 1), (2, 2), 1),     # weight-streaming regime, 18 pieces
    (134, 134, (31, 31), (3, 3), (1, 1), (1, 1), 6),    # 273 tiles: the serial multi-piece regime
    (64, 40, (6, 6), (3, 3), (0, 0), (1, 1), 1),        # one piece, no padding
]


def _gid(g):
    M, K, (H, W), (kh, kw), (ph, pw), (sh, sw), nb = g
    return f"M{M}-K{K}-{H}x{W}-k{kh}x{kw}-p{ph}{pw}-s{sh}{sw}-nb{nb}"


def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _out_hw(H, W, k, p, s):
    return (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1


def _tap_loop(t, taps, k, p, s):
    """Step 1 of the contract on the CPU in t's dtype: z from +0.0, z = z + taps[tap] * t over the
    taps in increasing order on the zero-padded input with strided slices (separate multiply and
    add; a padded position adds a zero of either sign, which leaves z's bits alone)."""
    (kh, kw), (ph, pw), (sh, sw) = k, p, s
    Ho, Wo = _out_hw(t.shape[2], t.shape[3], k, p, s)
    tp = F.pad(t, (pw, pw, ph, ph))
    z = torch.zeros(t.shape[0], t.shape[1], Ho, Wo, dtype=t.dtype)
    for a in range(kh):
        for b in range(kw):
            sl = tp[:, :, a:a + (Ho - 1) * sh + 1:sh, b:b + (Wo - 1) * sw + 1:sw]
            z = z + taps[a * kw + b][None, :, None, None] * sl
    return z


@functools.lru_cache(maxsize=None)
def _packed(shape, bits, scheme, seed=7):
    """(PackedTensor of a random tensor, its de-quantization) - computed once, never modified."""
    from admmq import quantize_packed
    p = quantize_packed([_randn(shape, seed + 131 * bits + shape[0], 0.3).to(DEV)], bits, scheme)[0]
    return p, p.dequantize()


@functools.lru_cache(maxsize=None)
def _inputs(g):
    """(t, taps, bias on the CPU, the same on the device, Z_ref on the CPU and on the device) of a
    geometry - computed once, shared by the tests, never modified."""
    M, K, (H, W), k, p, s, nb = g
    t, taps, bias = _randn((nb, K, H, W), 11 + K), _randn((k[0] * k[1], K), 12 + K, 0.5), _randn((M,), 13 + M)
    z = _tap_loop(t, taps, k, p, s)
    return dict(t=t, taps=taps, bias=bias, z=z, t_d=t.to(DEV), taps_d=taps.to(DEV), bias_d=bias.to(DEV), z_d=z.to(DEV))


def _fused(g, p, inp, bias):
    from admmq import packed_depthwise_conv1x1
    return packed_depthwise_conv1x1(inp["t_d"], inp["taps_d"], p, inp["bias_d"] if bias else None, kernel_size=g[3],
                                    stride=g[5], padding=g[4])


def _raw(p, g, t, taps, bias, y, ws=None, ws_bytes=None):
    """admmq_packed_dwgemm through ctypes on caller-owned buffers; returns the workspace size it reports."""
    from admmq import _lib
    from admmq.packed import _meta_words
    lib = _lib.load()
    M, K, (H, W), (kh, kw), (ph, pw), (sh, sw), nb = g
    Ho, Wo = _out_hw(H, W, g[3], g[4], g[5])
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    need = lib.admmq_packed_dwgemm_workspace_size(M, K, Ho, Wo, nb)
    if ws is None:
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
        ws_bytes = ws.numel()
    rc = lib.admmq_packed_dwgemm(_lib.ptr(p.codes), ctypes.byref(meta), M, K, _lib.ptr(t), nb, H, W, _lib.ptr(taps), kh, kw,
                                 sh, sw, ph, pw, _lib.ptr(bias), _lib.ptr(y), _lib.ptr(ws), ws_bytes, _lib.stream_handle(DEV))
    assert rc == 0, lib.admmq_last_error()
    torch.cuda.synchronize()
    return need


# --------------------------------------------------- 1. bit equality with the two-stage form
@pytest.mark.parametrize("g", GEOMS, ids=_gid)
def test_bit_equal_to_packed_conv1x1_of_the_tap_loop(g, monkeypatch):
    """With and without bias, through the torch op and through ctypes."""
    from admmq import _lib, packed_conv1x1
    M, K = g[0], g[1]
    p, _ = _packed((M, K), 4, MSE)
    inp = _inputs(g)
    for bias in (False, True):
        ref = packed_conv1x1(inp["z_d"], p, inp["bias_d"] if bias else None)
        y = _fused(g, p, inp, bias)
        assert y.shape == ref.shape and torch.equal(y, ref), (g, bias, "op")
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "use_ops", lambda: False)
            yc = _fused(g, p, inp, bias)
        assert torch.equal(yc, ref), (g, bias, "ctypes")


@pytest.mark.parametrize("bits,scheme", BITS_SCHEMES)
@pytest.mark.parametrize("g", GEOMS[:2], ids=_gid)
def test_bit_equal_over_bits_and_schemes(g, bits, scheme):
    from admmq import packed_conv1x1
    p, _ = _packed((g[0], g[1]), bits, scheme)
    inp = _inputs(g)
    for bias in (False, True):
        ref = packed_conv1x1(inp["z_d"], p, inp["bias_d"] if bias else None)
        assert torch.equal(_fused(g, p, inp, bias), ref), (g, bits, scheme, bias)


# --------------------------------------------------------------- 2. accuracy against float64
@pytest.mark.parametrize("g", GEOMS, ids=_gid)
def test_accuracy_against_float64(g):
    """|Y - Yd| <= (K + kh kw + 4) 2^-24 (|D| (|taps| * |t|) + |bias|) elementwise: a kh kw-term
    unfused inner product feeding a length-K float32 sum, to first order, with 2 units of slack
    for the second-order term (derived, not measured)."""
    M, K, _, k, pd, s, nb = g
    p, D = _packed((M, K), 4, MSE)
    inp = _inputs(g)
    D64 = D.double().cpu()
    zd = _tap_loop(inp["t"].double(), inp["taps"].double(), k, pd, s)
    zmag = _tap_loop(inp["t"].double().abs(), inp["taps"].double().abs(), k, pd, s)
    for bias in (False, True):
        y = _fused(g, p, inp, bias)
        yd = torch.einsum("mk,bkhw->bmhw", D64, zd)
        mag = torch.einsum("mk,bkhw->bmhw", D64.abs(), zmag)
        if bias:
            yd = yd + inp["bias"].double()[None, :, None, None]
            mag = mag + inp["bias"].double().abs()[None, :, None, None]
        err = (y.double().cpu() - yd).abs()
        bound = (K + k[0] * k[1] + 4) * U * mag
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f"dwgemm {_gid(g)} bias {bias}: max |err| / bound = {ratio:.4f}")
        assert torch.isfinite(y).all()
        assert bool((err <= bound).all()), f"{_gid(g)} bias {bias}: max |err| / bound = {ratio}"


# ------------------------------------------------------------------------ 3. stencil alone
def _selector(M, K):
    """An 8-bit tensor_symmetric PackedTensor [M, K] written by hand: scale 2^-6, code 128 -> 0.0,
    code 192 -> 1.0; row m holds its one 1.0 at column (5 m + 3) % K."""
    from admmq import PackedTensor
    codes = torch.full((M, K), 128, dtype=torch.uint8)
    sel = (5 * torch.arange(M) + 3) % K
    codes[torch.arange(M), sel] = 192
    p = PackedTensor(codes=codes.reshape(-1).to(DEV), shape=(M, K), bits=8, qscheme=SYM, scale=2.0 ** -6, zero_point=0,
                     mn=0.0, rng=0.0, index=-1)
    return p, sel


@pytest.mark.parametrize("g", GEOMS, ids=_gid)
def test_a_selecting_weight_returns_the_stencil(g):
    """Every output is one product by 1.0 plus exact zeros: Y[b, m] = Z_ref[b, sel(m)], bit for bit."""
    M, K = g[0], g[1]
    p, sel = _selector(M, K)
    D = p.dequantize().cpu()
    assert bool(((D != 0).sum(1) == 1).all()) and bool((D[torch.arange(M), sel] == 1.0).all())
    inp = _inputs(g)
    y = _fused(g, p, inp, False)
    assert torch.equal(y.cpu(), inp["z"][:, sel])


@pytest.mark.parametrize("g", GEOMS, ids=_gid)
def test_a_one_hot_centre_tap_gives_the_strided_1x1_conv(g):
    from admmq import packed_conv1x1, packed_depthwise_conv1x1
    M, K, (H, W), (kh, kw), (ph, pw), (sh, sw), nb = g
    p, _ = _packed((M, K), 4, MSE)
    inp = _inputs(g)
    Ho, Wo = _out_hw(H, W, g[3], g[4], g[5])
    a, b = kh // 2, kw // 2               # the tap at (a, b) reads t[oh sh - ph + a, ow sw - pw + b]
    taps = torch.zeros(kh * kw, K)
    taps[a * kw + b] = 1.0
    r0, c0 = a - ph, b - pw               # >= 0 for every geometry here: all its reads are inside the image
    assert r0 >= 0 and c0 >= 0 and r0 + (Ho - 1) * sh < H and c0 + (Wo - 1) * sw < W
    xs = inp["t_d"][:, :, r0:r0 + (Ho - 1) * sh + 1:sh, c0:c0 + (Wo - 1) * sw + 1:sw]
    y = packed_depthwise_conv1x1(inp["t_d"], taps.to(DEV), p, inp["bias_d"], kernel_size=g[3], stride=g[5], padding=g[4])
    assert torch.equal(y, packed_conv1x1(xs, p, inp["bias_d"]))


# ---------------------------------------------- 4. repeatability and batch independence
@pytest.mark.parametrize("g", [(64, 134, (7, 7), (3, 3), (1, 1), (1, 1), 3),        # parallel: 3 pieces, 3 tiles
                               (128, 1141, (4, 4), (3, 3), (1, 1), (2, 2), 3),      # parallel: 18 pieces
                               (134, 134, (31, 31), (3, 3), (1, 1), (1, 1), 6),     # serial, several pieces
                               (64, 40, (6, 6), (3, 3), (0, 0), (1, 1), 3)], ids=_gid)   # serial, one piece
def test_calls_repeat_and_images_do_not_depend_on_the_batch(g):
    from admmq import packed_depthwise_conv1x1
    p, _ = _packed((g[0], g[1]), 4, MSE)
    inp = _inputs(g)
    y1, y2 = _fused(g, p, inp, True), _fused(g, p, inp, True)
    assert torch.equal(y1, y2)
    for b in range(3):
        yb = packed_depthwise_conv1x1(inp["t_d"][b:b + 1].contiguous(), inp["taps_d"], p, inp["bias_d"], kernel_size=g[3],
                                      stride=g[5], padding=g[4])
        assert torch.equal(yb[0], y1[b]), (g, b)


# --------------------------------------------------------------------- 5. no stray writes
@pytest.mark.parametrize("g", [GEOMS[1], GEOMS[3], GEOMS[5], GEOMS[6], GEOMS[7]], ids=_gid)
def test_nothing_outside_the_output_or_the_workspace_is_written(g):
    """y and the workspace inside guard-banded buffers; t, taps and y 4 bytes past a 16-byte boundary."""
    from admmq import _lib
    M, K, (H, W), k, pd, s, nb = g
    p, _ = _packed((M, K), 4, MSE)
    inp = _inputs(g)
    Ho, Wo = _out_hw(H, W, k, pd, s)
    total = nb * M * Ho * Wo
    ref = _fused(g, p, inp, True)
    to = torch.empty(inp["t"].numel() + 1, device=DEV)[1:]
    po = torch.empty(inp["taps"].numel() + 1, device=DEV)[1:]
    to.copy_(inp["t_d"].reshape(-1))
    po.copy_(inp["taps_d"].reshape(-1))
    ybuf = torch.full((total + 129,), -12345.5, device=DEV)
    yv = ybuf[65:65 + total]
    assert to.data_ptr() % 16 == 4 and po.data_ptr() % 16 == 4 and yv.data_ptr() % 16 == 4
    need = _lib.load().admmq_packed_dwgemm_workspace_size(M, K, Ho, Wo, nb)
    assert need == _lib.load().admmq_packed_gemm_workspace_size(M, K, Ho * Wo, nb)
    ws = torch.full((256 + need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    _raw(p, g, to, po, inp["bias_d"], yv, ws=ws[256:], ws_bytes=need)
    assert bool((ybuf[:65] == -12345.5).all()) and bool((ybuf[65 + total:] == -12345.5).all())
    assert bool((ws[:256] == 0xA5).all()) and bool((ws[256 + need:] == 0xA5).all())
    assert torch.equal(yv.view(ref.shape), ref)
    assert torch.equal(to, inp["t_d"].reshape(-1)) and torch.equal(po, inp["taps_d"].reshape(-1))


# ------------------------------------------------------------------------------ 6. layer
def _rel_fro(y, y64):
    y64 = y64.detach()
    return float((y.detach().double().cpu() - y64).norm() / y64.norm())


def _factors(shapes, seed):
    from admmq import quantize_packed
    return quantize_packed([_randn(s, seed + i, 0.3).to(DEV) for i, s in enumerate(shapes)], 4, MSE)


@pytest.mark.parametrize("cout,cin,k,R,stride", [(64, 64, 3, 134, 1), (128, 64, 3, 70, 2)])
def test_fused_factorized_conv(cout, cin, k, R, stride, tmp_path):
    from admmq import export
    conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=True).to(DEV)
    shapes = [(cout, R), (cin, R), (k * k, R)]
    pf = _factors(shapes, 30)
    seq = export.factorized_conv(conv, R, pf, fused=True)
    plain = export.factorized_conv(conv, R, pf)
    assert [n for n, _ in seq.named_children()] == ["conv1", "conv23"]
    assert [n for n, _ in plain.named_children()] == ["conv1", "conv2", "conv3"]
    m = seq.conv23
    assert type(seq.conv1) is export.PackedConv1x1 and seq.conv1.transpose
    assert type(m) is export.PackedDepthwiseConv1x1 and isinstance(m, export._PackedWeight) and not hasattr(m, "weight")
    assert (m.out_features, m.in_features, m.kernel_size, m.stride, m.padding) == \
        (cout, R, (k, k), (stride, stride), (k // 2, k // 2))
    assert m.codes.dtype == torch.uint8 and m.codes.numel() == cout * R // 2
    deq = [p.dequantize() for p in pf]
    assert m.taps.dtype == torch.float32 and torch.equal(m.taps, deq[2])
    x = _randn((2, cin, 8, 8), 31).to(DEV)
    y = seq(x)
    # the unfused packed layer with its conv2 replaced by the float32 tap loop: the same bits
    t1 = plain.conv1(x)
    z = _tap_loop(t1.cpu(), deq[2].cpu(), (k, k), (k // 2, k // 2), (stride, stride))
    assert torch.equal(y, plain.conv3(z.to(DEV)))
    # ... and the distance to the float64 layer that the unfused packed layer's test asserts
    ref = export.factorized_conv(conv.cpu(), R, [d.cpu() for d in deq]).double()
    conv.to(DEV)
    y64 = ref(x.double().cpu())
    rel = _rel_fro(y, y64)
    print(f"fused factorized_conv {(cout, cin, k, R, stride)}: rel Frobenius {rel:.3e}")
    assert y.shape == y64.shape and rel <= 1e-5
    # state_dict -> torch.save -> a fresh fused layer (other codes, other taps) -> the same bits
    path = str(tmp_path / "layer.pt")
    torch.save(seq.state_dict(), path)
    fresh = export.factorized_conv(conv, R, _factors(shapes, 77), fused=True)
    assert not torch.equal(fresh(x), y)
    fresh.load_state_dict(torch.load(path, map_location=DEV, weights_only=True))
    assert torch.equal(fresh(x), y)
    # inference only
    with pytest.raises(RuntimeError, match="inference only"):
        seq.conv23(t1.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="inference only"):
        seq(x.clone().requires_grad_())
    from admmq import _lib
    from admmq.packed import _meta_words
    with pytest.raises(RuntimeError, match="inference only"):
        _lib.ops().packed_dwgemm(pf[0].codes, _meta_words(pf[0]), cout, R, t1.clone().requires_grad_(), m.taps, k, k,
                                 stride, stride, k // 2, k // 2, None)
    with torch.no_grad():
        assert torch.equal(seq(x.clone().requires_grad_()), y)


def test_torch_compile_of_the_fused_layer_runs():
    from admmq import export
    cout, cin, k, R = 64, 64, 3, 134
    conv = nn.Conv2d(cin, cout, k, padding=1, bias=True).to(DEV)
    seq = export.factorized_conv(conv, R, _factors([(cout, R), (cin, R), (k * k, R)], 30), fused=True)
    x = _randn((2, cin, 8, 8), 31).to(DEV)
    with torch.no_grad():
        y = torch.compile(seq)(x)
        assert torch.equal(y, seq(x))
