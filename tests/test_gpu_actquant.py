"""Fixed-range activation quantizers on the MI355X. Every comparison is bit
equality. k_fixed_quant against the reference's formula evaluated step by step in float32 on
the CPU (including the half-way points of every level moved by -2..+2 ulps, NaN, +-inf, -0.0,
values far outside the range, rng == 0 and rng < 0, and a misaligned input); the packed GEMM's
output quantizer against fixed_quantize of the plain call in both regimes; the fused stage's
mid quantizer against packed_conv1x1 on the quantized tap-loop Z (a quantized padding element
would show: 0 is not on the mid grid); nothing outside the output and the workspace is written.
The stand-alone functions and the observers are compared with the golden fixture F12, written
by the reference's own functions on the CPU, as uint32 views: no element is exempt, NaNs included."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE = "tensor_mseminmax_symmetric"
DEV = torch.device("cuda:0")
MID = (4, 0.3, 0.3 + 1.1)      # bits, min, max: mn = 0.3, rng = fl32(1.1) - q(0) != 0


def _u32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _fixture():
    """The golden fixture F12 (tests/golden/gen_f12_actquant.py): the reference's own functions on the CPU."""
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "f12_actquant.json")) as f:
        cases = json.load(f)["cases"]
    return cases, np.load(os.path.join(here, "f12_actquant.npz"))


def _expected(arrays, cid):
    return torch.from_numpy(arrays["out_" + cid].view(np.int32).copy())


def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _specials(n, seed):
    x = _randn((n,), seed, 2.0)
    sp = [float("nan"), float("inf"), -float("inf"), -0.0, 0.0, 1e30, -1e30, 1e-40]
    for i, v in enumerate(sp[:n]):
        x[(i * 7) % n] = v
    return x


# ------------------------------------------------------------------ 1. stand-alone functions
def _run_case(c, x):
    from admmq import fixed_quantize, min_max_quantize
    if c["kind"] in ("fixed", "boundary"):
        return fixed_quantize(x, c["bits"], c["zero_point"], c["scope"])
    if c["kind"] == "one_none":
        return min_max_quantize(x, c["bits"], None, 1.0)
    lo = torch.tensor(c["min"], dtype=torch.float32, device=DEV) if c["route"] in ("tensor", "mixed_tf") else c["min"]
    hi = torch.tensor(c["max"], dtype=torch.float32) if c["route"] in ("tensor", "mixed_ft") else c["max"]   # (a CPU bound too)
    return min_max_quantize(x, c["bits"], lo, hi)


@pytest.mark.parametrize("route", ["op", "ctypes"])
def test_functions_match_the_reference_bit_for_bit(route, monkeypatch):
    """Every function and boundary case of F12: uint32 views, no element exempt. The input sits 4 bytes
    past a 16-byte boundary for the large size."""
    from admmq import _lib
    cases, arrays = _fixture()
    if route == "ctypes":
        monkeypatch.setattr(_lib, "use_ops", lambda: False)
    dev = {}
    for k in arrays.files:
        if k.startswith("in_") and k != "in_obs":
            x = torch.from_numpy(arrays[k])
            buf = torch.empty(x.numel() + 1, device=DEV)
            dev[k[3:]] = buf[1:].copy_(x) if x.numel() > 1000 else x.to(DEV)
    assert dev["x4099"].data_ptr() % 16 == 4
    n = 0
    bad = []
    for c in cases:
        if c["kind"] == "observer":
            continue
        y = _run_case(c, dev[c["input"]])
        if not torch.equal(_u32(y), _expected(arrays, c["id"])):
            bad.append((c["id"], int((_u32(y) != _expected(arrays, c["id"])).sum())))
        n += 1
    print(f"F12 {route}: {n} cases, {len(bad)} differ: {bad[:12]}")
    assert n >= 200 and not bad, bad


def test_output_alignment_and_guard_bands():
    """y aligned like x (vectors behind a head of 3) and differently (all scalar), inside guard bands."""
    from admmq import _lib
    from admmq.quantization import act_record
    cases, arrays = _fixture()
    c = next(c for c in cases if c["id"] == "fx_b8_n4099_r0")
    x = torch.from_numpy(arrays["in_x4099"])
    xv = torch.empty(4100, device=DEV)[1:].copy_(x)
    q = act_record(8, float(np.float32(c["zero_point"])), float(np.float32(c["scope"])))
    for yoff in (1, 2):
        ybuf = torch.full((4099 + 8,), -7.25, device=DEV)
        yv = ybuf[yoff:yoff + 4099]
        rc = _lib.load().admmq_fixed_quantize(_lib.ptr(xv), _lib.ptr(yv), 4099, ctypes.byref(q), _lib.stream_handle(DEV))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(_u32(yv), _expected(arrays, c["id"])), yoff
        assert bool((ybuf[:yoff] == -7.25).all()) and bool((ybuf[yoff + 4099:] == -7.25).all())


# ------------------------------------------------------------------------------ 2. observers
@pytest.mark.parametrize("ltype", ["minmax", "avgminmax"])
def test_observers_match_the_reference(ltype):
    """min_val / max_val after each observed batch (kept on the device) and the first quantizing output."""
    from admmq import actquant
    cases, arrays = _fixture()
    c = next(c for c in cases if c["kind"] == "observer" and c["ltype"] == ltype)
    batches = torch.from_numpy(arrays["in_obs"]).to(DEV)
    q = actquant.get_quant_layer(ltype, "s", bits=c["bits"], counter=c["counter"])
    for b, (lo, hi) in zip(batches[:3], c["stats_bits"]):
        assert q(b) is b
        assert q.min_val.device.type == "cuda" and q.min_val.dim() == 0 and q.min_val.dtype == torch.float32
        assert int(_u32(q.min_val.reshape(1))[0]) == np.uint32(lo).view(np.int32)
        assert int(_u32(q.max_val.reshape(1))[0]) == np.uint32(hi).view(np.int32)
    assert q.counter == 0
    y = q(batches[3])
    assert y.shape == batches[3].shape and torch.equal(_u32(y).reshape(-1), _expected(arrays, c["id"]).reshape(-1))


# ------------------------------------------------------------------------------ 3. epilogue
@functools.lru_cache(maxsize=None)
def _packed(shape, bits=4, scheme=MSE, seed=7):
    from admmq import quantize_packed
    return quantize_packed([_randn(shape, seed + 131 * bits + shape[0], 0.3).to(DEV)], bits, scheme)[0]


def _quartile_act(y):
    """An 8 bit range from the quartiles of the unquantized output: values fall inside and outside."""
    q = torch.quantile(y.detach().float().cpu().reshape(-1)[:100000], torch.tensor([0.25, 0.75]))
    return (8, float(q[0]), float(q[1]))


# (M, K, N, nb): parallel pieces + k_packed_reduce; one piece, serial; M / K / C tails; serial, several pieces
CONV_SHAPES = [(64, 134, 49, 3), (134, 64, 65, 2), (33, 65, 70, 1), (134, 134, 961, 6)]


@pytest.mark.parametrize("route", ["op", "ctypes"])
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "M%d-K%d-N%d-nb%d" % s)
def test_epilogue_conv1x1(shape, trans, route, monkeypatch):
    from admmq import _lib, fixed_quantize, min_max_quantize, packed_conv1x1
    if route == "ctypes":
        monkeypatch.setattr(_lib, "use_ops", lambda: False)
    M, K, N, nb = shape
    p = _packed((K, M) if trans else (M, K))
    x = _randn((nb, K, 1, N), 3 + M).to(DEV)
    bias = _randn((M,), 4 + M).to(DEV)
    regime = _lib.load().admmq_packed_gemm_workspace_size(M, K, N, nb) > 0
    assert regime == (shape in (CONV_SHAPES[0], CONV_SHAPES[2]))   # several K pieces on few tiles: the parallel form
    for b in (None, bias):
        plain = packed_conv1x1(x, p, b, transpose=trans)
        assert torch.equal(packed_conv1x1(x, p, b, transpose=trans, act=None), plain)
        for act in (MID, _quartile_act(plain)):
            ref = min_max_quantize(plain, *act)
            y = packed_conv1x1(x, p, b, transpose=trans, act=act)
            assert torch.equal(y, ref), (shape, trans, b is not None, act)
            assert not torch.equal(y, plain)
    assert torch.equal(fixed_quantize(plain, 4, 0.3, float(np.float32(1.4) - np.float32(0.3))),
                       min_max_quantize(plain, 4, torch.tensor(0.3), 1.4))   # mixed bounds: float32 first


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("mk", [(64, 134), (134, 64)])
def test_epilogue_linear(mk, trans):
    from admmq import min_max_quantize, packed_linear
    M, K = mk
    p = _packed((K, M) if trans else (M, K))
    x = _randn((70, K), 8 + M).to(DEV)
    bias = _randn((M,), 4 + M).to(DEV)
    for b in (None, bias):
        plain = packed_linear(x, p, b, transpose=trans)
        for act in (MID, _quartile_act(plain)):
            assert torch.equal(packed_linear(x, p, b, transpose=trans, act=act), min_max_quantize(plain, *act)), (mk, trans, act)


def test_quantizer_off_gives_the_existing_call():
    """on = 0 and NULL through the C entry point."""
    from admmq import _lib, packed_conv1x1
    from admmq.packed import _meta_words
    M, K, N, nb = CONV_SHAPES[0]
    p = _packed((M, K))
    x = _randn((nb, K, 7, 7), 3 + M).to(DEV)
    plain = packed_conv1x1(x, p)
    lib = _lib.load()
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    need = lib.admmq_packed_gemm_workspace_size(M, K, N, nb)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    off = _lib.ActQ(4, 0, 0.3, 1.1)
    for q in (None, ctypes.byref(off)):
        y = torch.empty_like(plain)
        rc = lib.admmq_packed_gemm_act(_lib.ptr(p.codes), ctypes.byref(meta), 0, M, K, _lib.ptr(x), 0, N, nb, None,
                                       _lib.ptr(y), q, _lib.ptr(ws), ws.numel(), _lib.stream_handle(DEV))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(y, plain)


# --------------------------------------------------------------------------- 4. fused stage
# (M, K, (H, W), (kh, kw), (ph, pw), (sh, sw), nb): GEOMS[0], [1], [5], [6], [7] of test_gpu_packed_dwgemm.py
GEOMS = [
    (64, 134, (7, 7), (3, 3), (1, 1), (1, 1), 3),
    (33, 65, (8, 8), (3, 3), (1, 1), (2, 2), 2),
    (128, 1141, (4, 4), (3, 3), (1, 1), (2, 2), 1),
    (134, 134, (31, 31), (3, 3), (1, 1), (1, 1), 6),
    (64, 40, (6, 6), (3, 3), (0, 0), (1, 1), 1),
]


def _gid(g):
    M, K, (H, W), (kh, kw), (ph, pw), (sh, sw), nb = g
    return f"M{M}-K{K}-{H}x{W}-k{kh}x{kw}-p{ph}{pw}-s{sh}{sw}-nb{nb}"


def _out_hw(H, W, k, p, s):
    return (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1


def _tap_loop(t, taps, k, p, s):
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
def _inputs(g):
    M, K, (H, W), k, p, s, nb = g
    t, taps, bias = _randn((nb, K, H, W), 11 + K), _randn((k[0] * k[1], K), 12 + K, 0.5), _randn((M,), 13 + M)
    z = _tap_loop(t, taps, k, p, s)
    return dict(t_d=t.to(DEV), taps_d=taps.to(DEV), bias_d=bias.to(DEV), z_d=z.to(DEV))


@pytest.mark.parametrize("route", ["op", "ctypes"])
@pytest.mark.parametrize("g", GEOMS, ids=_gid)
def test_fused_stage_mid_and_output_quantizers(g, route, monkeypatch):
    from admmq import _lib, min_max_quantize, packed_conv1x1, packed_depthwise_conv1x1
    if route == "ctypes":
        monkeypatch.setattr(_lib, "use_ops", lambda: False)
    M, K = g[0], g[1]
    p = _packed((M, K))
    inp = _inputs(g)
    zq = min_max_quantize(inp["z_d"], *MID)
    for bias in (None, inp["bias_d"]):
        plain_mid = packed_conv1x1(zq, p, bias)
        plain = packed_conv1x1(inp["z_d"], p, bias)
        out = _quartile_act(plain)
        kw = dict(kernel_size=g[3], stride=g[5], padding=g[4])
        fused = lambda **q: packed_depthwise_conv1x1(inp["t_d"], inp["taps_d"], p, bias, **kw, **q)
        assert torch.equal(fused(), plain)
        assert torch.equal(fused(mid_act=MID), plain_mid), (g, "mid")
        assert torch.equal(fused(act=out), min_max_quantize(plain, *out)), (g, "out")
        assert torch.equal(fused(mid_act=MID, act=out), min_max_quantize(plain_mid, *out)), (g, "both")
        assert not torch.equal(plain_mid, plain)


# ----------------------------------------------------------------------- 5. no stray writes
@pytest.mark.parametrize("g", [GEOMS[1], GEOMS[2]], ids=_gid)
def test_fused_stage_writes_nothing_outside(g):
    from admmq import _lib, packed_depthwise_conv1x1
    from admmq.packed import _meta_words
    from admmq.quantization import act_range, act_record
    M, K, (H, W), (kh, kw), (ph, pw), (sh, sw), nb = g
    p = _packed((M, K))
    inp = _inputs(g)
    Ho, Wo = _out_hw(H, W, g[3], g[4], g[5])
    total = nb * M * Ho * Wo
    out = (8, -0.5, 0.75)
    ref = packed_depthwise_conv1x1(inp["t_d"], inp["taps_d"], p, inp["bias_d"], kernel_size=g[3], stride=g[5], padding=g[4],
                                   mid_act=MID, act=out)
    lib = _lib.load()
    need = lib.admmq_packed_dwgemm_workspace_size(M, K, Ho, Wo, nb)
    ybuf = torch.full((total + 129,), -12345.5, device=DEV)
    yv = ybuf[65:65 + total]
    ws = torch.full((256 + need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    mq, oq = act_record(MID[0], *act_range(*MID[1:])), act_record(out[0], *act_range(*out[1:]))
    rc = lib.admmq_packed_dwgemm_act(_lib.ptr(p.codes), ctypes.byref(meta), M, K, _lib.ptr(inp["t_d"]), nb, H, W,
                                     _lib.ptr(inp["taps_d"]), kh, kw, sh, sw, ph, pw, _lib.ptr(inp["bias_d"]), _lib.ptr(yv),
                                     ctypes.byref(mq), ctypes.byref(oq), _lib.ptr(ws[256:]), need, _lib.stream_handle(DEV))
    assert rc == 0, lib.admmq_last_error()
    torch.cuda.synchronize()
    assert bool((ybuf[:65] == -12345.5).all()) and bool((ybuf[65 + total:] == -12345.5).all())
    assert bool((ws[:256] == 0xA5).all()) and bool((ws[256 + need:] == 0xA5).all())
    assert torch.equal(yv.view(ref.shape), ref)


def test_epilogue_writes_nothing_outside():
    from admmq import _lib, packed_conv1x1
    from admmq.packed import _meta_words
    from admmq.quantization import act_range, act_record
    M, K, N, nb = CONV_SHAPES[0]
    p = _packed((M, K))
    x = _randn((nb, K, 7, 7), 3 + M).to(DEV)
    bias = _randn((M,), 4 + M).to(DEV)
    ref = packed_conv1x1(x, p, bias, act=MID)
    lib = _lib.load()
    total = nb * M * N
    need = lib.admmq_packed_gemm_workspace_size(M, K, N, nb)
    assert need > 0
    ybuf = torch.full((total + 129,), -12345.5, device=DEV)
    yv = ybuf[65:65 + total]
    ws = torch.full((256 + need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    oq = act_record(MID[0], *act_range(*MID[1:]))
    rc = lib.admmq_packed_gemm_act(_lib.ptr(p.codes), ctypes.byref(meta), 0, M, K, _lib.ptr(x), 0, N, nb, _lib.ptr(bias),
                                   _lib.ptr(yv), ctypes.byref(oq), _lib.ptr(ws[256:]), need, _lib.stream_handle(DEV))
    assert rc == 0, lib.admmq_last_error()
    torch.cuda.synchronize()
    assert bool((ybuf[:65] == -12345.5).all()) and bool((ybuf[65 + total:] == -12345.5).all())
    assert bool((ws[:256] == 0xA5).all()) and bool((ws[256 + need:] == 0xA5).all())
    assert torch.equal(yv.view(ref.shape), ref)


# -------------------------------------------------------------------------------- 6. layers
def _factors(shapes, seed):
    from admmq import quantize_packed
    return quantize_packed([_randn(s, seed + i, 0.3).to(DEV) for i, s in enumerate(shapes)], 4, MSE)


@pytest.mark.parametrize("cout,cin,k,R,stride", [(64, 64, 3, 134, 1), (128, 64, 3, 70, 2)])
def test_factorized_conv_with_activation_quantizers(cout, cin, k, R, stride, tmp_path):
    """The calibrated add_quant-wrapped packed layer, the fused layer and the unfused layer built with
    act_quant= give the same bits. The unfused forms are evaluated stage by stage with the depthwise
    nn.Conv2d replaced by the float32 tap loop (the fused kernel's contract; the library's depthwise
    kernel sums in another order), each with its own quantizers."""
    from torch import nn
    from admmq import actquant, export
    conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=True).to(DEV)
    shapes = [(cout, R), (cin, R), (k * k, R)]
    pf = _factors(shapes, 30)
    taps = pf[2].dequantize().cpu()
    geom = ((k, k), (k // 2, k // 2), (stride, stride))
    wrapped = export.factorized_conv(conv, R, pf)
    for name in ("conv1", "conv2", "conv3"):
        setattr(wrapped, name, actquant.add_quant(name, getattr(wrapped, name), "minmax", bits=8, counter=4))
    with torch.no_grad():
        for seed in (41, 42):   # two batches of 2: the counter reaches 0
            wrapped(_randn((2, cin, 8, 8), seed).to(DEV))
    assert all(getattr(wrapped, n).activation_post_process.counter == 0 for n in ("conv1", "conv2", "conv3"))
    acts = actquant.collect(wrapped)
    assert len(acts) == 3 and all(a is not None and a[0] == 8 and a[1] < a[2] for a in acts)
    fused = export.factorized_conv(conv, R, pf, fused=True, act_quant=acts)
    unfused = export.factorized_conv(conv, R, pf, act_quant=acts)
    assert fused.conv23._mid_act is not None and fused.conv23._act is not None and fused.conv1._act is not None
    assert type(unfused.conv2.activation_post_process) is actquant.FixedQuant

    def staged(layer, conv1, post2, conv3, x):
        t1 = conv1(x)
        z = _tap_loop(t1.cpu(), taps, *geom).to(DEV)
        return conv3(post2(z))

    x = _randn((2, cin, 8, 8), 43).to(DEV)
    with torch.no_grad():
        y = fused(x)
        ya = staged(wrapped, wrapped.conv1, wrapped.conv2.activation_post_process, wrapped.conv3, x)
        yc = staged(unfused, unfused.conv1, unfused.conv2.activation_post_process, unfused.conv3, x)
        plain = export.factorized_conv(conv, R, pf, fused=True)(x)
    assert torch.equal(y, ya) and torch.equal(y, yc) and not torch.equal(y, plain)
    # state_dict -> torch.save -> a fresh fused layer without quantizers -> the same bits
    path = str(tmp_path / "layer.pt")
    torch.save(fused.state_dict(), path)
    fresh = export.factorized_conv(conv, R, _factors(shapes, 77), fused=True)
    fresh.load_state_dict(torch.load(path, map_location=DEV, weights_only=True))
    with torch.no_grad():
        assert torch.equal(fresh(x), y)
        assert torch.equal(torch.compile(fused)(x), y)
    with pytest.raises(RuntimeError, match="inference only"):
        fused(x.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="inference only"):
        unfused.conv1(x.clone().requires_grad_())


def test_ops_refuse_an_input_that_requires_grad():
    from admmq import _lib
    from admmq.packed import _meta_words
    p = _packed((64, 134))
    x = _randn((1, 134, 4, 4), 2).to(DEV).requires_grad_(True)
    ops = _lib.ops()
    with pytest.raises(RuntimeError, match="inference only"):
        ops.packed_gemm_act(p.codes, _meta_words(p), False, 64, 134, x, 0, None, 4, 0.3, 1.1)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.fixed_quantize(x, 4, 0.3, 1.1)
    taps = _randn((9, 134), 3).to(DEV)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.packed_dwgemm_act(p.codes, _meta_words(p), 64, 134, x, taps, 3, 3, 1, 1, 1, 1, None, 4, 0.3, 1.1, 0, 0.0, 0.0)


def test_inference_only():
    from admmq import packed_conv1x1
    p = _packed((64, 134))
    x = _randn((1, 134, 4, 4), 2).to(DEV).requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        packed_conv1x1(x, p, act=MID)
    with torch.no_grad():
        assert packed_conv1x1(x, p, act=MID).shape == (1, 64, 4, 4)
