"""Half-precision fused depthwise + 1x1 stage on the MI355X: k_packed_hdwgemm returns
the bits of the half packed_conv1x1 on a Z_h formed by the float32 tap loop on the CPU and rounded once
to the input's type, meets a derived bound against float64, touches nothing outside its output and its
workspace, and the fused export layer runs end to end on half inputs."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE, MINMAX, SYM, AFF = "tensor_mseminmax_symmetric", "tensor_minmax", "tensor_symmetric", "tensor_affine"
DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16]
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DT = {torch.float16: 1, torch.bfloat16: 2}

# (M, K, (H, W), (kh, kw), (ph, pw), (sh, sw), nb)
GEOMS = [
    (64, 134, (7, 7), (3, 3), (1, 1), (1, 1), 3),       # columns cross image boundaries inside a tile; K tail; 3 pieces
    (33, 65, (8, 8), (3, 3), (1, 1), (2, 2), 2),        # M tail, stride
    (40, 70, (5, 9), (1, 3), (0, 1), (1, 2), 1),        # asymmetric window
    (64, 134, (9, 9), (5, 5), (2, 2), (1, 1), 1),       # 25 taps
    (128, 1141, (4, 4), (3, 3), (1, 1), (2, 2), 1),     # weight-streaming regime, 18 pieces
    (134, 134, (31, 31), (3, 3), (1, 1), (1, 1), 6),    # serial regime, three row tiles: a 6-row second block, a row-tile tail
    (64, 40, (6, 6), (3, 3), (0, 0), (1, 1), 1),        # one piece, no padding
]


def _gid(g):
    M, K, (H, W), (kh, kw), (ph, pw), (sh, sw), nb = g
    return f"M{M}-K{K}-{H}x{W}-k{kh}x{kw}-p{ph}{pw}-s{sh}{sw}-nb{nb}"


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _out_hw(g):
    _, _, (H, W), k, p, s, _ = g
    return (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1


def _tap_loop(t, taps, g):
    """Step 1 of the contract on the CPU in t's dtype: z from +0.0, z = z + taps[tap] * t over the taps in
    increasing order on the zero-padded input (a padded position adds a zero, which leaves z's bits alone)."""
    (kh, kw), (ph, pw), (sh, sw) = g[3], g[4], g[5]
    Ho, Wo = _out_hw(g)
    tp = F.pad(t, (pw, pw, ph, ph))
    z = torch.zeros(t.shape[0], t.shape[1], Ho, Wo, dtype=t.dtype)
    for a in range(kh):
        for b in range(kw):
            z = z + taps[a * kw + b][None, :, None, None] * tp[:, :, a:a + (Ho - 1) * sh + 1:sh, b:b + (Wo - 1) * sw + 1:sw]
    return z


@functools.lru_cache(maxsize=None)
def _packed(shape, bits, scheme):
    """(PackedTensor of a random tensor, its de-quantization) - computed once, never modified."""
    from admmq import quantize_packed
    p = quantize_packed([_randn(shape, 7 + 131 * bits + shape[0], 0.3).to(DEV)], bits, scheme)[0]
    return p, p.dequantize()


@functools.lru_cache(maxsize=None)
def _inputs(g, dtype):
    """The half t, float32 taps and bias of a geometry and Z_h = the float32 tap loop over t.float(), rounded once
    to dtype - computed once, shared by the tests, never modified."""
    M, K, (H, W), k, _, _, nb = g
    t = _randn((nb, K, H, W), 11 + K).to(dtype)
    taps, bias = _randn((k[0] * k[1], K), 12 + K, 0.5), _randn((M,), 13 + M)
    zh = _tap_loop(t.float(), taps, g).to(dtype)
    return dict(t=t, taps=taps, bias=bias, t_d=t.to(DEV), taps_d=taps.to(DEV), bias_d=bias.to(DEV), zh_d=zh.to(DEV))


def _fused(g, p, inp, bias, out_dtype=None):
    from admmq import packed_depthwise_conv1x1
    return packed_depthwise_conv1x1(inp["t_d"], inp["taps_d"], p, inp["bias_d"] if bias else None, kernel_size=g[3],
                                    stride=g[5], padding=g[4], out_dtype=out_dtype)


def _check_equal(g, p, inp, what):
    from admmq import packed_conv1x1
    for bias in (False, True):
        for od in (None, torch.float32):
            ref = packed_conv1x1(inp["zh_d"], p, inp["bias_d"] if bias else None, out_dtype=od)
            y = _fused(g, p, inp, bias, od)
            assert y.dtype == ref.dtype and y.shape == ref.shape and torch.equal(y, ref), (what, bias, od)


# --------------------------------------------------- 1. bit equality with the two-stage form
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("g", GEOMS, ids=_gid)
def test_bit_equal_to_the_half_packed_conv1x1_of_the_rounded_tap_loop(g, dtype, monkeypatch):
    from admmq import _lib
    p, _ = _packed((g[0], g[1]), 4, MSE)
    inp = _inputs(g, dtype)
    _check_equal(g, p, inp, "op")
    if g is GEOMS[0]:
        assert torch.equal(_fused(g, p, inp, True), _fused(g, p, inp, True))   # results repeat
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "use_ops", lambda: False)
            _check_equal(g, p, inp, "ctypes")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("bits,scheme", [(3, AFF), (4, MSE), (8, MINMAX), (4, SYM), (1, SYM)])
@pytest.mark.parametrize("g", GEOMS[:2], ids=_gid)
def test_bit_equal_over_bits_and_schemes(g, bits, scheme, dtype):
    _check_equal(g, _packed((g[0], g[1]), bits, scheme)[0], _inputs(g, dtype), (bits, scheme))


# --------------------------------------------------------------- 2. bound against float64
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("bits,scheme", [(4, MSE), (8, MINMAX)])
@pytest.mark.parametrize("g", GEOMS, ids=_gid)
def test_bound_against_float64(g, bits, scheme, dtype):
    """|Y - Yd| <= B = (u + (K + kh kw + 6) 2^-23) mag elementwise for the float32 result, mag = |D| (|taps| * |t|) +
    |bias| (tensor_minmax: |D - mn| + |mn| for |D|, as the half GEMM's bound), u = 2^-8 (bf16) / 2^-11 (fp16): one
    rounding of z to the half type, a kh kw-term unfused float32 sum, a K-term float32 sum at a full ulp per add, and
    the epilogue. The half result: B + u (|Yd| + B). Derived, not measured (largest err / bound seen: 0.21 / 0.35)."""
    M, K, _, k, _, _, _ = g
    p, D = _packed((M, K), bits, scheme)
    inp = _inputs(g, dtype)
    u = UNIT[dtype]
    D64 = D.double().cpu()
    Dmag = (D64 - p.mn).abs() + abs(p.mn) if scheme == MINMAX else D64.abs()
    yd = torch.einsum("mk,bkhw->bmhw", D64, _tap_loop(inp["t"].double(), inp["taps"].double(), g))
    yd = yd + inp["bias"].double()[None, :, None, None]
    mag = torch.einsum("mk,bkhw->bmhw", Dmag, _tap_loop(inp["t"].double().abs(), inp["taps"].double().abs(), g))
    mag = mag + inp["bias"].double().abs()[None, :, None, None]
    B = (u + (K + k[0] * k[1] + 6) * 2.0 ** -23) * mag
    for od, bound in ((torch.float32, B), (None, B + u * (yd.abs() + B))):
        y = _fused(g, p, inp, True, od)
        err = (y.double().cpu() - yd).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f"hdwgemm {_gid(g)} {dtype} {scheme} out {y.dtype}: max |err| / bound = {ratio:.4f}")
        assert torch.isfinite(y).all() and bool((err <= bound).all()), ratio


# --------------------------------------------------------------------- 3. no stray writes
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("g", [GEOMS[0], GEOMS[5]], ids=_gid)
def test_nothing_outside_the_output_or_the_workspace_is_written(g, dtype, out_f32):
    """admmq_packed_hdwgemm through ctypes; y and the workspace are cut out of larger buffers filled with a sentinel."""
    from admmq import _lib
    from admmq.packed import _meta_words
    lib = _lib.load()
    M, K, (H, W), (kh, kw), (ph, pw), (sh, sw), nb = g
    p, _ = _packed((M, K), 4, MSE)
    inp = _inputs(g, dtype)
    Ho, Wo = _out_hw(g)
    total = nb * M * Ho * Wo
    ref = _fused(g, p, inp, True, torch.float32 if out_f32 else None)
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    need = lib.admmq_packed_hdwgemm_workspace_size(ctypes.byref(meta), M, K, Ho, Wo, nb)
    assert need == lib.admmq_packed_hgemm_workspace_size(ctypes.byref(meta), M, K, Ho * Wo, nb)
    ybuf = torch.full((total + 130,), -12345.5, dtype=ref.dtype, device=DEV)
    yv = ybuf[65:65 + total]
    ws = torch.full((256 + need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = lib.admmq_packed_hdwgemm(_lib.ptr(p.codes), ctypes.byref(meta), M, K, _lib.ptr(inp["t_d"]), DT[dtype], nb, H, W,
                                  _lib.ptr(inp["taps_d"]), kh, kw, sh, sw, ph, pw, _lib.ptr(inp["bias_d"]), _lib.ptr(yv),
                                  0 if out_f32 else DT[dtype], _lib.ptr(ws[256:]), need, _lib.stream_handle(DEV))
    assert rc == 0, lib.admmq_last_error()
    torch.cuda.synchronize()
    assert bool((ybuf[:65] == -12345.5).all()) and bool((ybuf[65 + total:] == -12345.5).all())
    assert bool((ws[:256] == 0xA5).all()) and bool((ws[256 + need:] == 0xA5).all())
    assert torch.equal(yv.view(ref.shape), ref)


# ------------------------------------------------------------------------------ 4. layer
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cout,cin,k,R,stride", [(64, 64, 3, 134, 1), (128, 64, 3, 70, 2)])
def test_fused_cp_layer_on_half_inputs(cout, cin, k, R, stride, dtype, tmp_path):
    from admmq import export, packed_conv1x1, quantize_packed
    shapes = [(cout, R), (cin, R), (k * k, R)]
    pf = quantize_packed([_randn(s, 30 + i, 0.3).to(DEV) for i, s in enumerate(shapes)], 4, MSE)
    bias = _randn((cout,), 29).to(DEV)
    args = (cin, cout, (k, k), k // 2, stride)
    seq = export.build_cp_layer(R, pf, bias, *args, fused=True)
    g = (cout, R, (8, 8), (k, k), (k // 2, k // 2), (stride, stride), 2)
    x = _randn((2, cin, 8, 8), 31).to(DEV).to(dtype)
    for cast in (False, True):   # float32 taps and bias, then the module's own half ones
        if cast:
            seq = seq.to(dtype)
            assert seq.conv23.taps.dtype == dtype and seq.conv23.codes.dtype == torch.uint8
        y = seq(x)
        assert y.dtype == dtype and tuple(y.shape) == (2, cout) + _out_hw(g)   # the unfused layout's shape
        t1 = seq.conv1(x)
        zh = _tap_loop(t1.float().cpu(), seq.conv23.taps.float().cpu(), g).to(dtype).to(DEV)
        assert torch.equal(seq.conv23(t1), packed_conv1x1(zh, pf[0], seq.conv23.bias))
        assert torch.equal(y, seq.conv23(t1))
    if cast:
        assert seq.conv23._taps_f32() is seq.conv23._taps_f32()   # one float32 copy, no cast per forward
    path = str(tmp_path / "layer.pt")
    torch.save(seq.state_dict(), path)
    fresh = export.build_cp_layer(R, quantize_packed([_randn(s, 77 + i, 0.3).to(DEV) for i, s in enumerate(shapes)], 4, MSE),
                                  bias, *args, fused=True).to(dtype)
    assert not torch.equal(fresh(x), y)
    fresh.load_state_dict(torch.load(path, map_location=DEV, weights_only=True))
    assert torch.equal(fresh(x), y)
    for setter in (seq.conv23.set_activation_quant, seq.conv23.set_mid_activation_quant):
        setter(4, -1.0, 1.0)
        with pytest.raises(ValueError, match="act="):
            seq(x)
        setter(None)
