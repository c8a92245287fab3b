"""Integer fused depthwise + 1x1 stage on the MI355X: k_packed_idwgemm equals the
numpy oracle bit for bit - int64 tap sums D / Cv by explicit window loops, the contract's double
formula for z, the float32 restatement of encode for its codes, then the integer GEMM's oracle -
for every weight width, geometry, tap scheme, quantizer width and regime; its clamp counters equal
the oracle's counts; it equals the chain through packed_conv1x1_int on the oracle's codes; it
writes nothing outside its outputs; packed_taps_int is the integer factor zero padded; and the
3-way integer layer equals the chain of functional calls, round-trips through its state dict and
sits closer to the float packed layer than that layer's own quantization noise."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from torch import nn

from conftest import gpu_available
import test_gpu_packed_igemm as ig   # the igemm test's helpers: _np_levels, its oracle, cached packed weights

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE, SYM, AFF = ig.MSE, ig.SYM, ig.AFF
DEV = ig.DEV
TMN, TRNG = ig.XMN, ig.XRNG   # t_q = (bits, -0.7, 2.3): mn_t != 0, so a wrong Cv shows


def _out_hw(H, W, ks, st, pd):
    return (H + 2 * pd[0] - ks[0]) // st[0] + 1, (W + 2 * pd[1] - ks[1]) // st[1] + 1


def _stencil(c, ut, ks, st, pd):
    """int64 D, Cv [nb, K, Ho, Wo]: explicit loops over the output positions and the window."""
    nb, K, H, W = ut.shape
    Ho, Wo = _out_hw(H, W, ks, st, pd)
    u = ut.astype(np.int64)
    D = np.zeros((nb, K, Ho, Wo), np.int64)
    Cv = np.zeros((nb, K, Ho, Wo), np.int64)
    for oh in range(Ho):
        for ow in range(Wo):
            for a in range(ks[0]):
                for b in range(ks[1]):
                    ih, iw = oh * st[0] - pd[0] + a, ow * st[1] - pd[1] + b
                    if 0 <= ih < H and 0 <= iw < W:
                        D[:, :, oh, ow] += c[a * ks[1] + b][None, :] * u[:, :, ih, iw]
                        Cv[:, :, oh, ow] += c[a * ks[1] + b][None, :]
    return D, Cv


def _z(D, Cv, s_c, tbits):
    """The contract's double formula, one rounding to float32."""
    g = np.float64(np.float32(TRNG)) / np.float64((1 << tbits) - 1)
    return (np.float64(np.float32(s_c)) * (g * D.astype(np.float64) + np.float64(np.float32(TMN)) * Cv.astype(np.float64))
            ).astype(np.float32)


def _encode(z, bits, mn, rng):
    """(codes uint8, number clamped): the float32 restatement of act_encode."""
    qi, n = ig._np_levels(z, bits, mn, rng)
    bad = ~((qi >= 0) & (qi <= n))
    return np.where(np.isnan(qi), 0, np.clip(qi, 0, n)).astype(np.uint8), int(bad.sum())


def _range(lo, hi):
    from admmq.quantization import act_range
    return act_range(lo, hi)


def _rec(bits, mn, rng):
    from admmq import _lib
    return _lib.ActQ(int(bits), 1, float(mn), float(rng))


@functools.lru_cache(maxsize=None)
def _case(M, K, abits, nb, H, W, ks, st, pd, cbits=4, cscheme=MSE, tbits=8, mbits=6, shrink=1.0, seed=0):
    """One shape's inputs and oracle, made once: dict(p, C, ut, bias, mid, uz, nclamp, ref)."""
    p, a = ig._weight((M, K), abits, MSE)
    C, c = ig._weight((ks[0] * ks[1], K), cbits, cscheme)
    ut = ig._codes((nb, K, H, W), tbits, 2000 + seed + 7 * K + H)
    bias = ig._randn((M,), 2001 + M)
    D, Cv = _stencil(c, ut.cpu().numpy(), ks, st, pd)
    assert int(np.abs(D).max()) <= 49 * 128 * 255
    z = _z(D, Cv, C.scale, tbits)
    lo, hi = float(z.min()), float(z.max())
    mn, rng = _range(shrink * lo - (0.05 if shrink == 1.0 else 0.0), shrink * hi + (0.05 if shrink == 1.0 else 0.0))
    uz, nclamp = _encode(z, mbits, mn, rng)
    Ho, Wo = z.shape[2:]
    ref = ig._oracle_layout(a, uz.reshape(nb, K, Ho * Wo), 0, p.scale, mbits, mn, rng, bias).reshape(nb, M, Ho, Wo)
    return dict(p=p, C=C, ut=ut, bias=bias, mid=(mbits, mn, rng), uz=uz, nclamp=nclamp, numel=z.size, ref=ref, tbits=tbits,
                geom=(ks, st, pd))


def _call(cs, act=None, out_codes=False, ut=None, bias="case"):
    from admmq import packed_depthwise_conv1x1_int
    ks, st, pd = cs["geom"]
    xq = ig._xq(cs["ut"] if ut is None else ut, cs["tbits"], TMN, TRNG)
    return packed_depthwise_conv1x1_int(xq, cs["C"], cs["p"], ks, st, pd, cs["bias"] if bias == "case" else bias,
                                        _rec(*cs["mid"]), act, out_codes, return_mid_clamped=True)


def _check_float(cs, what):
    y, midc = _call(cs)
    assert y.dtype == torch.float32 and tuple(y.shape) == cs["ref"].shape, what
    assert ig._bits_equal(y, cs["ref"]), what
    assert int(midc) == cs["nclamp"], what
    return y


# --------------------------------------------------------------------------- widths
@pytest.mark.parametrize("abits", range(1, 9))
def test_every_weight_width_and_output_form(abits):
    """M = 65, K = 70 (a tile tail in M, one full K step and a tail of 6), 3 images of 5 x 5 under a 3 x 3
    window with pad 1: 75 columns - two column tiles, a tile that spans images, a column tail."""
    from admmq import act_encode, fixed_quantize
    cs = _case(65, 70, abits, 3, 5, 5, (3, 3), (1, 1), (1, 1))
    y = _check_float(cs, abits)
    assert cs["nclamp"] == 0
    lo, hi = float(y.min()), float(y.max())
    for act in [(6, lo - 0.1, hi + 0.1), (3, 0.25 * lo, 0.25 * hi)]:
        mn, rng = _range(act[1], act[2])
        yq, _ = _call(cs, act)
        assert torch.equal(yq.view(torch.int32), fixed_quantize(y, act[0], mn, rng).view(torch.int32)), (abits, act)
        got, _ = _call(cs, act, out_codes=True)
        want = act_encode(y, act, check=False)
        assert got.codes.dtype == torch.uint8 and got.codes.shape == y.shape
        assert (got.bits, got.mn, got.rng) == (want.bits, want.mn, want.rng)
        assert torch.equal(got.codes, want.codes), (abits, act)
        assert int(got.clamped) == int(want.clamped) and (int(got.clamped) > 0) == (act[0] == 3)
    y0, _ = _call(cs, bias=None)
    from admmq import packed_depthwise_conv1x1_int
    yn = packed_depthwise_conv1x1_int(ig._xq(cs["ut"], 8, TMN, TRNG), cs["C"], cs["p"], (3, 3), 1, 1, None, _rec(*cs["mid"]))
    assert torch.equal(yn.view(torch.int32), y0.view(torch.int32))   # the counter not asked for: the same bits
    ref0 = ig._oracle_layout(ig._weight((65, 70), abits, MSE)[1], cs["uz"].reshape(3, 70, 25), 0, cs["p"].scale, cs["mid"][0],
                             cs["mid"][1], cs["mid"][2], None).reshape(3, 65, 5, 5)
    assert ig._bits_equal(y0, ref0)


# ------------------------------------------------------------------------- geometry
GEOMETRY = [
    # M, K, nb, H, W, kernel, stride, padding
    (65, 70, 2, 7, 6, (3, 3), (2, 2), (1, 1)),     # stride 2
    (65, 70, 2, 5, 6, (1, 3), (1, 1), (0, 1)),
    (65, 70, 2, 6, 5, (3, 1), (1, 1), (1, 0)),
    (33, 70, 3, 5, 5, (7, 7), (1, 1), (3, 3)),     # the window overhangs on both sides at once
    (65, 70, 3, 5, 5, (3, 3), (1, 1), (0, 0)),     # no padding
    (65, 1, 3, 5, 5, (3, 3), (1, 1), (1, 1)),      # K = 1
    (65, 64, 3, 5, 5, (3, 3), (1, 1), (1, 1)),     # K = 64 exactly: one full step, no tail
    (33, 70, 2, 6, 7, (3, 5), (2, 1), (1, 2)),     # unequal kernel, stride and padding
]


@pytest.mark.parametrize("g", GEOMETRY, ids=[str(i) for i in range(len(GEOMETRY))])
def test_geometry(g):
    M, K, nb, H, W, ks, st, pd = g
    _check_float(_case(M, K, 4, nb, H, W, ks, st, pd), g)


# ------------------------------------------------------------------- taps and widths
@pytest.mark.parametrize("cbits,cscheme", [(b, s) for b in (2, 4, 8) for s in (MSE, SYM, AFF)])
def test_tap_schemes_and_quantizer_widths(cbits, cscheme):
    """C at 2, 4, 8 bits under the three schemes (8-bit affine in the igemm test's int8-fitting range)
    x t bits {2, 5, 8} x mid bits {2, 8}."""
    for tbits in (2, 5, 8):
        for mbits in (2, 8):
            cs = _case(65, 70, 4, 3, 5, 5, (3, 3), (1, 1), (1, 1), cbits, cscheme, tbits, mbits)
            _check_float(cs, (cbits, cscheme, tbits, mbits))


# -------------------------------------------------------------------------- regimes
PARALLEL = (65, 130, 4, 3, 5, 5, (3, 3), (1, 1), (1, 1))       # few tiles: three K pieces + k_packed_ireduce
SERIAL = (256, 130, 4, 4, 32, 32, (3, 3), (1, 1), (1, 1))      # 4 x 64 = 256 tiles: one workgroup per tile over all of K


@pytest.mark.parametrize("shape,parallel", [(PARALLEL, True), (SERIAL, False)], ids=["parallel", "serial"])
def test_both_regimes_equal_the_oracle(shape, parallel):
    from admmq import _lib
    M, K, _, nb, H, W, ks, st, pd = shape
    Ho, Wo = _out_hw(H, W, ks, st, pd)
    lib = _lib.load()
    need = lib.admmq_packed_idwgemm_workspace_size(M, K, Ho, Wo, nb)
    assert need == lib.admmq_packed_igemm_workspace_size(M, K, Ho * Wo, nb) and (need > 0) == parallel
    if parallel:
        assert need == 3 * nb * M * Ho * Wo * 4
    cs = _case(*shape)
    y = _check_float(cs, shape)
    y2, _ = _call(cs)
    assert torch.equal(y2.view(torch.int32), y.view(torch.int32))   # two calls: the same bits
    if parallel:   # one image per call: the same bits as the batched call (here both run the parallel regime)
        for b in range(nb):
            yb, _ = _call(cs, ut=cs["ut"][b:b + 1].contiguous())
            assert torch.equal(yb[0].view(torch.int32), y[b].view(torch.int32)), b
    else:          # one image of the serial shape runs the parallel regime (64 tiles): the same bits again
        assert lib.admmq_packed_idwgemm_workspace_size(M, K, Ho, Wo, 1) > 0
        yb, _ = _call(cs, ut=cs["ut"][1:2].contiguous())
        assert torch.equal(yb[0].view(torch.int32), y[1].view(torch.int32))


# ------------------------------------------------------------------------- counters
@pytest.mark.parametrize("shape", [PARALLEL, SERIAL], ids=["parallel", "serial"])
def test_clamp_counters(shape):
    """M > 64 in both regimes: an element of Z is staged by every row tile (and, in the parallel regime,
    its K piece), and counts once. A covering range counts 0; half the range clamps some but not all."""
    from admmq import act_encode
    cov = _case(*shape)
    assert cov["nclamp"] == 0
    _check_float(cov, "covering")
    cs = _case(*shape, shrink=0.5)
    assert 0 < cs["nclamp"] < cs["numel"]
    y = _check_float(cs, "clamping")
    act = (5, 0.5 * float(y.min()), 0.5 * float(y.max()))
    got, midc = _call(cs, act, out_codes=True)
    want = act_encode(y, act, check=False)
    assert torch.equal(got.codes, want.codes)
    assert int(got.clamped) == int(want.clamped) > 0
    assert int(midc) == cs["nclamp"]


# ---------------------------------------------------------------------------- chain
def test_equals_the_chain_through_packed_conv1x1_int():
    from admmq import QuantizedActivation, packed_conv1x1_int
    for shape in (PARALLEL, (65, 70, 4, 2, 7, 6, (3, 3), (2, 2), (1, 1))):
        cs = _case(*shape)
        y, _ = _call(cs)
        uz = QuantizedActivation(torch.from_numpy(cs["uz"]).to(DEV), *cs["mid"])
        assert torch.equal(y.view(torch.int32), packed_conv1x1_int(uz, cs["p"], cs["bias"]).view(torch.int32))
        act = (6, float(y.min()) - 0.1, float(y.max()) + 0.1)
        got, _ = _call(cs, act, out_codes=True)
        assert torch.equal(got.codes, packed_conv1x1_int(uz, cs["p"], cs["bias"], act=act, out_codes=True).codes)


# ------------------------------------------------------------ nothing else is touched
@pytest.mark.parametrize("shape", [PARALLEL, (65, 70, 4, 3, 5, 5, (3, 3), (1, 1), (1, 1)), SERIAL],
                         ids=["parallel", "small", "serial"])
def test_nothing_outside_the_outputs_or_the_workspace_is_touched(shape):
    """admmq_packed_idwgemm on caller-owned buffers: guard values around y / y_codes, behind the workspace and
    around both counters; t's codes at an odd address."""
    from admmq import _lib, packed_rowsums, packed_taps_int
    from admmq.packed import _meta_words
    lib = _lib.load()
    cs = _case(*shape)
    M, K, _, nb, H, W, ks, st, pd = shape
    Ho, Wo = _out_hw(H, W, ks, st, pd)
    total = nb * M * Ho * Wo
    p, C = cs["p"], cs["C"]
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    need = lib.admmq_packed_idwgemm_workspace_size(M, K, Ho, Wo, nb)
    tbuf = torch.full((cs["ut"].numel() + 32,), 0x5A, dtype=torch.uint8, device=DEV)
    to = tbuf[1:1 + cs["ut"].numel()]
    to.copy_(cs["ut"].reshape(-1))
    assert to.data_ptr() % 2 == 1
    tq, mq = _rec(cs["tbits"], TMN, TRNG), _rec(*cs["mid"])
    omn, orng = _range(float(cs["ref"].min()) - 0.1, float(cs["ref"].max()) + 0.1)
    oq = _rec(6, omn, orng)
    want_codes, _ = _encode(cs["ref"], 6, omn, orng)

    def raw(y, yc, out, midc, outc, ws):
        rc = lib.admmq_packed_idwgemm(_lib.ptr(p.codes), ctypes.byref(meta), M, K, _lib.ptr(to), ctypes.byref(tq), nb, H, W,
                                      _lib.ptr(packed_taps_int(C)), float(C.scale), ks[0], ks[1], st[0], st[1], pd[0], pd[1],
                                      _lib.ptr(packed_rowsums(p)), _lib.ptr(cs["bias"]), _lib.ptr(y), _lib.ptr(yc),
                                      ctypes.byref(mq), ctypes.byref(out) if out is not None else None, _lib.ptr(midc),
                                      _lib.ptr(outc), _lib.ptr(ws), ws.numel(), _lib.stream_handle(DEV))
        assert rc == 0, lib.admmq_last_error()
        torch.cuda.synchronize()

    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    ybuf = torch.full((total + 128,), -12345.5, device=DEV)
    cnt = torch.full((5,), 99, dtype=torch.int32, device=DEV)
    raw(ybuf[64:64 + total], None, None, cnt[1:2], None, ws)
    assert bool((ybuf[:64] == -12345.5).all()) and bool((ybuf[64 + total:] == -12345.5).all())
    assert ig._bits_equal(ybuf[64:64 + total].view(cs["ref"].shape), cs["ref"])
    assert cnt.tolist() == [99, 0, 99, 99, 99]
    ycb = torch.full((total + 128,), 0xC3, dtype=torch.uint8, device=DEV)
    raw(None, ycb[61:61 + total], oq, cnt[1:2], cnt[3:4], ws)
    assert bool((ycb[:61] == 0xC3).all()) and bool((ycb[61 + total:] == 0xC3).all())
    assert np.array_equal(ycb[61:61 + total].view(cs["ref"].shape).cpu().numpy(), want_codes)
    assert cnt.tolist() == [99, 0, 99, 0, 99]
    assert bool((ws[need:] == 0xA5).all())
    assert bool((tbuf[:1] == 0x5A).all()) and bool((tbuf[1 + cs["ut"].numel():] == 0x5A).all())
    # both counters may be NULL
    raw(ybuf[64:64 + total], None, None, None, None, ws)
    assert ig._bits_equal(ybuf[64:64 + total].view(cs["ref"].shape), cs["ref"])


# ------------------------------------------------------------------------ tap image
@pytest.mark.parametrize("K", [1, 63, 64, 70])
def test_packed_taps_int_is_the_integer_factor_zero_padded(K):
    from admmq import packed_taps_int
    from admmq.packed import taps_kp
    for bits, scheme, ntaps in [(4, MSE, 9), (8, AFF, 9), (2, SYM, 49), (5, AFF, 3)]:
        C, c = ig._weight((ntaps, K), bits, scheme)
        img = packed_taps_int(C)
        Kp = taps_kp(K)
        assert Kp % 64 == 0 and K <= Kp < K + 64
        assert img.dtype == torch.int8 and tuple(img.shape) == (ntaps, Kp)
        got = img.cpu().numpy().astype(np.int64)
        assert np.array_equal(got[:, :K], c), (K, bits, scheme)
        assert not got[:, K:].any()
        assert packed_taps_int(C) is img   # kept on the packed tensor


# --------------------------------------------------------------------------- layers
def _cp_factors(cout, cin, R, ks, seed, bits=4):
    from admmq import quantize_packed
    return quantize_packed([ig._randn(s, seed + i, 0.3) for i, s in enumerate([(cout, R), (cin, R), (ks[0] * ks[1], R)])],
                           bits, MSE)


@pytest.mark.parametrize("stride", [1, 2])
def test_cp_integer_layer(tmp_path, stride):
    from admmq import act_encode, export, fixed_quantize, packed_conv1x1_int, packed_depthwise_conv1x1_int
    cout, cin, R, ks = 70, 24, 40, (3, 3)
    pf = _cp_factors(cout, cin, R, ks, 50)
    bias = ig._randn((cout,), 51)
    x = ig._randn((2, cin, 7, 6), 52).clamp_(-3.9, 3.9)
    in_act = (8, -4.0, 4.0)

    def build(factors=None, **kw):
        return export.build_cp_layer(R, pf if factors is None else factors, bias, cin, cout, ks, 1, stride, **kw)

    plain = build()                      # conv1 / conv2 / conv3, no quantizers
    assert [n for n, _ in plain.named_children()] == ["conv1", "conv2", "conv3"]
    with torch.no_grad():
        h = plain.conv1(x)
        z = plain.conv2(h)
        y_plain = plain.conv3(z)
    acts = [(8, float(h.min()) - 0.05, float(h.max()) + 0.05), (6, float(z.min()) - 0.05, float(z.max()) + 0.05),
            (8, float(y_plain.min()) - 0.05, float(y_plain.max()) + 0.05)]
    layer = build(act_quant=acts, integer=True, in_act=in_act)
    assert type(layer) is export.IntegerPackedCP and [n for n, _ in layer.named_children()] == ["conv1", "conv23"]
    assert type(layer.conv1) is export.PackedConv1x1 and type(layer.conv23) is export.PackedDepthwiseConv1x1
    with torch.no_grad():
        y = layer(x)
        assert y.dtype == torch.float32 and y.shape == y_plain.shape
        # the chain of functional calls
        xq = act_encode(x, in_act)
        hq = packed_conv1x1_int(xq, pf[1], None, True, 1, acts[0], out_codes=True)
        yf = packed_depthwise_conv1x1_int(hq, pf[2], pf[0], ks, stride, 1, bias, acts[1], acts[2])
        assert torch.equal(y.view(torch.int32), yf.view(torch.int32))
        assert len(layer.last_clamped) == 3 and [int(c) for c in layer.last_clamped] == [0, 0, 0]
        # without the output quantizer: a float output, the functional call's bits
        l2 = build(act_quant=acts[:2] + [None], integer=True, in_act=in_act)
        assert torch.equal(l2(x).view(torch.int32),
                           packed_depthwise_conv1x1_int(hq, pf[2], pf[0], ks, stride, 1, bias, acts[1]).view(torch.int32))
        # codes out: four counters
        layer.out_codes = True
        yc = layer(x)
        layer.out_codes = False
        assert len(layer.last_clamped) == 4 and int(layer.last_clamped[3]) == 0
        assert torch.equal(yc.dequantize().view(torch.int32), y.view(torch.int32))
        # state dict -> file -> a fresh layer built from other factors and quantizers
        path = str(tmp_path / "int_cp_layer.pt")
        torch.save(layer.state_dict(), path)
        other = _cp_factors(cout, cin, R, ks, 90)

        def fresh():
            return build(factors=other, act_quant=[(5, -1.0, 1.0), (4, -1.0, 1.0), None], integer=True, in_act=(4, -1.0, 1.0))

        f1 = fresh()
        assert not torch.equal(f1(x), y)
        f1.load_state_dict(torch.load(path, map_location=DEV, weights_only=True))
        assert torch.equal(f1(x).view(torch.int32), y.view(torch.int32))
        # a state without the row sums and the tap image rebuilds them
        sd = torch.load(path, map_location=DEV, weights_only=True)
        sd["_extra_state"] = dict(sd["_extra_state"], rowsums=None, taps_i8=None)
        f2 = fresh()
        f2.load_state_dict(sd)
        assert torch.equal(f2(x).view(torch.int32), y.view(torch.int32))
        assert torch.equal(f2._taps(), layer._taps())
        # a wrong shape or dtype is refused
        for key, bad in [("taps_i8", torch.zeros(9, 40, dtype=torch.int8)), ("taps_i8", torch.zeros(9, 64)),
                         ("rowsums", [torch.zeros(R + 1, dtype=torch.int32), None]),
                         ("rowsums", [None, torch.zeros(cout)])]:
            sd["_extra_state"] = dict(torch.load(path, weights_only=True)["_extra_state"], **{key: bad})
            with pytest.raises(ValueError, match="integer layer state"):
                fresh().load_state_dict(sd)
        # closeness: the float packed fused layer with the same quantizers on the same quantized input
        mn, rng = _range(in_act[1], in_act[2])
        fl = build(fused=True, act_quant=acts)
        y_fl = fl(fixed_quantize(x, in_act[0], mn, rng))
        d_int, d_q = ig._rel(y, y_fl), ig._rel(y_fl, y_plain)
        print(f"integer CP layer vs float packed fused layer with quantizers: {d_int:.3e}; that layer vs unquantized: "
              f"{d_q:.3e}")
        assert d_int < d_q
        # the same without the output quantizer (its grid hides differences below half a step)
        fl2 = build(fused=True, act_quant=acts[:2] + [None])
        y2, y_fl2 = l2(x), fl2(fixed_quantize(x, in_act[0], mn, rng))
        d_int2, d_q2 = ig._rel(y2, y_fl2), ig._rel(y_fl2, y_plain)
        print(f"without the output quantizer: {d_int2:.3e}; {d_q2:.3e}")
        assert d_int2 < d_q2
        # compiled module containing the integer layer
        if stride == 1:
            assert torch.equal(torch.compile(nn.Sequential(layer))(x), y)


def test_factorized_conv_builds_the_integer_layer():
    from admmq import export
    cout, cin, R, ks = 70, 24, 40, (3, 3)
    pf = _cp_factors(cout, cin, R, ks, 50)
    conv = nn.Conv2d(cin, cout, ks, stride=2, padding=1, bias=True, device=DEV)
    acts = [(8, -3.0, 3.0), (6, -3.0, 3.0), None]
    layer = export.factorized_conv(conv, R, pf, act_quant=acts, integer=True, in_act=(8, -4.0, 4.0))
    assert type(layer) is export.IntegerPackedCP and layer.conv23.stride == (2, 2) and layer.conv23.padding == (1, 1)
    x = ig._randn((1, cin, 6, 6), 53).clamp_(-3.9, 3.9)
    with torch.no_grad():
        same = export.build_cp_layer(R, pf, conv.bias.detach(), cin, cout, ks, conv.padding, conv.stride, act_quant=acts,
                                     integer=True, in_act=(8, -4.0, 4.0))
        assert torch.equal(layer(x).view(torch.int32), same(x).view(torch.int32))
    assert type(export.factorized_conv(conv, R, pf)) is nn.Sequential


def test_ctypes_route_equals_the_op_route(monkeypatch):
    from admmq import _lib
    from admmq.packed import _meta_words, _taps_i8
    cs = _case(65, 70, 4, 3, 5, 5, (3, 3), (1, 1), (1, 1))
    act = (5, 0.5 * float(cs["ref"].min()), 0.5 * float(cs["ref"].max()))

    def run():
        y, m1 = _call(cs)
        q, m2 = _call(cs, act, out_codes=True)
        return y, m1, q.codes, q.clamped, m2, _taps_i8(cs["C"].codes, _meta_words(cs["C"]), 9, 70)

    ops = run()
    monkeypatch.setattr(_lib, "use_ops", lambda: False)
    raw = run()
    assert int(ops[3]) > 0
    for i, (o, r) in enumerate(zip(ops, raw)):
        assert o.dtype == r.dtype and torch.equal(o.view(torch.uint8) if o.dtype == torch.float32 else o,
                                                  r.view(torch.uint8) if r.dtype == torch.float32 else r), i


def test_op_refuses_a_bias_that_requires_grad():
    from admmq import _lib, packed_rowsums, packed_taps_int
    from admmq.packed import _meta_words
    cs = _case(65, 70, 4, 3, 5, 5, (3, 3), (1, 1), (1, 1))
    p, C = cs["p"], cs["C"]
    b = cs["bias"].clone().requires_grad_()
    args = (p.codes, _meta_words(p), 65, 70, cs["ut"], 8, TMN, TRNG, packed_taps_int(C), float(C.scale), 3, 3, 1, 1, 1, 1,
            packed_rowsums(p), b, cs["mid"][0], cs["mid"][1], cs["mid"][2], 0, 0.0, 0.0, False, True)
    with pytest.raises(RuntimeError, match="inference only"):
        _lib.ops().packed_idwgemm(*args)
    with torch.no_grad():
        y, midc, outc = _lib.ops().packed_idwgemm(*args)
    assert ig._bits_equal(y, cs["ref"]) and int(midc) == 0 and outc.numel() == 0
