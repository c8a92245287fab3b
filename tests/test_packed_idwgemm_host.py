"""Integer fused depthwise + 1x1 stage, host side (no GPU): the exports exist, every refusal of the
new entry points comes back with its documented status and its own error text before any device
call (made-up device addresses), the workspace size equals the integer GEMM's over a grid of
arguments, the tap image's size is ntaps * 64 ceil(K / 64), the Meta kernels give the right shapes
and dtypes, and the Python wrappers and the 3-way builder check their arguments on the host."""
import ctypes

import pytest
import torch

OK, ERR_ARG, ERR_WORKSPACE, ERR_SCHEME = 0, -1, -3, -4
MSE, MINMAX, SYMMETRIC, AFFINE = 0, 1, 2, 3
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    return _lib.load()


def _meta(scheme=MSE, bits=4, bad=0, zp=0):
    from admmq import _lib
    return _lib.QMeta(scheme, bits, 0.125, zp, 0.0, 1.0, -1, bad)


def _actq(bits=8, on=1):
    from admmq import _lib
    return _lib.ActQ(bits, on, -1.0, 2.0)


def test_exports_exist(lib):
    for name in ("admmq_packed_taps_i8_bytes", "admmq_packed_taps_i8", "admmq_packed_idwgemm_workspace_size",
                 "admmq_packed_idwgemm"):
        assert hasattr(lib, name), name
    import admmq
    from admmq import export
    assert callable(admmq.packed_taps_int) and callable(admmq.packed_depthwise_conv1x1_int)
    assert issubclass(export.IntegerPackedCP, torch.nn.Module)


def _call(lib, meta="ok", codes=0x1000, t=0x10001, tq="ok", taps=0x70000, rs=0x30000, y=0x20000, yc=0, mid="ok", out=None,
          midc=0, clamped=0, M=8, K=8, nb=1, H=5, W=5, k=(3, 3), s=(1, 1), p=(1, 1), bias=0, ws=0x100000, ws_bytes=1 << 20):
    m = _meta() if meta == "ok" else meta
    q = _actq() if tq == "ok" else tq
    mq = _actq(6) if mid == "ok" else mid
    return lib.admmq_packed_idwgemm(P(codes), ctypes.byref(m) if m is not None else None, M, K, P(t),
                                    ctypes.byref(q) if q is not None else None, nb, H, W, P(taps), 0.125, k[0], k[1], s[0],
                                    s[1], p[0], p[1], P(rs), P(bias), P(y), P(yc), ctypes.byref(mq) if mq is not None else None,
                                    ctypes.byref(out) if out is not None else None, P(midc), P(clamped), P(ws), ws_bytes,
                                    None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(codes=0), ERR_ARG, b"NULL"),
    (dict(t=0), ERR_ARG, b"NULL"),
    (dict(meta=None), ERR_ARG, b"NULL"),
    (dict(rs=0), ERR_ARG, b"NULL"),
    (dict(tq=None), ERR_ARG, b"NULL"),
    (dict(taps=0), ERR_ARG, b"NULL"),
    (dict(y=0), ERR_ARG, b"exactly one"),
    (dict(yc=0x40000), ERR_ARG, b"exactly one"),
    (dict(M=0), ERR_ARG, b"positive"),
    (dict(K=-3), ERR_ARG, b"positive"),
    (dict(H=0), ERR_ARG, b"positive"),
    (dict(W=0), ERR_ARG, b"positive"),
    (dict(nb=0), ERR_ARG, b"positive"),
    (dict(meta=(MSE, 0)), ERR_ARG, b"bits"),
    (dict(meta=(SYMMETRIC, 9)), ERR_ARG, b"bits"),
    (dict(meta=(4, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(MINMAX, 4)), ERR_SCHEME, b"tensor_minmax"),
    (dict(meta=(AFFINE, 4, 2)), ERR_ARG, b"bad"),
    (dict(meta=(AFFINE, 8, 0, 1)), ERR_ARG, b"int8"),
    (dict(meta=(AFFINE, 8, 0, -1)), ERR_ARG, b"int8"),
    (dict(K=65537), ERR_ARG, b"65536"),
    (dict(tq=(1,)), ERR_ARG, b"t_q"),
    (dict(tq=(9,)), ERR_ARG, b"t_q"),
    (dict(tq=(8, 0)), ERR_ARG, b"t_q"),
    (dict(mid=None), ERR_ARG, b"mid_q"),               # the mid quantizer is mandatory
    (dict(mid=(6, 0)), ERR_ARG, b"mid_q"),
    (dict(mid=(1,)), ERR_ARG, b"mid_q"),
    (dict(mid=(9,)), ERR_ARG, b"mid_q"),
    (dict(y=0, yc=0x40001), ERR_ARG, b"codes output"),                 # no out_q
    (dict(y=0, yc=0x40001, out=(9,)), ERR_ARG, b"codes output"),
    (dict(out=(25,)), ERR_ARG, b"1..24"),
    (dict(k=(0, 3)), ERR_ARG, b"kernel size"),
    (dict(k=(3, 8)), ERR_ARG, b"kernel size"),
    (dict(s=(0, 1)), ERR_ARG, b"stride"),
    (dict(p=(3, 1)), ERR_ARG, b"padding"),
    (dict(p=(1, -1)), ERR_ARG, b"padding"),
    (dict(H=2, W=2, k=(5, 5), p=(1, 1)), ERR_ARG, b"does not fit"),
    (dict(codes=0x1004), ERR_ARG, b"16-byte"),
    (dict(taps=0x70008), ERR_ARG, b"taps_i8 must be 16-byte"),
    (dict(y=0x20002), ERR_ARG, b"aligned"),
    (dict(bias=0x50001), ERR_ARG, b"aligned"),
    (dict(rs=0x30002), ERR_ARG, b"aligned"),
    (dict(midc=0x60002), ERR_ARG, b"aligned"),
    (dict(y=0, yc=0x40001, out=(6,), clamped=0x60002), ERR_ARG, b"aligned"),
    (dict(M=1 << 30), ERR_ARG, b"range"),
    (dict(K=65536, H=1 << 12, W=1 << 12, nb=2), ERR_ARG, b"2^40"),
    (dict(M=512, K=1141, H=2, W=2, ws_bytes=16), ERR_WORKSPACE, b"workspace"),
    (dict(M=512, K=1141, H=2, W=2, ws=0, ws_bytes=1 << 30), ERR_WORKSPACE, b"workspace"),
])
def test_packed_idwgemm_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    for k in ("tq", "mid", "out"):
        if isinstance(kw.get(k), tuple):
            kw[k] = _actq(*kw[k])
    assert _call(lib, **kw) == status
    assert word in lib.admmq_last_error(), lib.admmq_last_error()


def test_allowed_records_pass_the_checks(lib):
    """What is allowed gets past every argument check: the next refusal is the short workspace."""
    for bits, zp in [(8, 0), (7, 63), (7, -64), (4, -8), (1, 0)]:
        assert _call(lib, meta=_meta(AFFINE, bits, 0, zp), M=512, K=1141, H=2, W=2, ws_bytes=16) == ERR_WORKSPACE
    for k, s, p, H, W in [((7, 7), (1, 1), (6, 6), 1, 1), ((1, 1), (3, 2), (0, 0), 2, 2), ((3, 5), (2, 1), (1, 2), 2, 3)]:
        assert _call(lib, M=512, K=1141, H=H, W=W, k=k, s=s, p=p, ws_bytes=16) == ERR_WORKSPACE, (k, s, p)
    for tb, mb in [(2, 2), (8, 8), (2, 8)]:
        assert _call(lib, tq=_actq(tb), mid=_actq(mb), M=512, K=1141, H=2, W=2, ws_bytes=16) == ERR_WORKSPACE


def test_taps_i8_refusals_and_size(lib):
    m = _meta()
    f = lib.admmq_packed_taps_i8
    for args, status, word in [
        ((P(0), ctypes.byref(m), 9, 8, P(0x2000), None), ERR_ARG, b"NULL"),
        ((P(0x1000), None, 9, 8, P(0x2000), None), ERR_ARG, b"NULL"),
        ((P(0x1000), ctypes.byref(m), 9, 8, P(0), None), ERR_ARG, b"NULL"),
        ((P(0x1000), ctypes.byref(m), 0, 8, P(0x2000), None), ERR_ARG, b"positive"),
        ((P(0x1000), ctypes.byref(m), 9, 0, P(0x2000), None), ERR_ARG, b"positive"),
        ((P(0x1000), ctypes.byref(m), 50, 8, P(0x2000), None), ERR_ARG, b"49"),
        ((P(0x1000), ctypes.byref(_meta(MINMAX, 4)), 9, 8, P(0x2000), None), ERR_SCHEME, b"tensor_minmax"),
        ((P(0x1000), ctypes.byref(_meta(AFFINE, 8, 0, 5)), 9, 8, P(0x2000), None), ERR_ARG, b"int8"),
        ((P(0x1000), ctypes.byref(_meta(MSE, 4, 3)), 9, 8, P(0x2000), None), ERR_ARG, b"bad"),
        ((P(0x1000), ctypes.byref(_meta(MSE, 9)), 9, 8, P(0x2000), None), ERR_ARG, b"bits"),
        ((P(0x1000), ctypes.byref(m), 9, 65537, P(0x2000), None), ERR_ARG, b"65536"),
        ((P(0x1008), ctypes.byref(m), 9, 8, P(0x2000), None), ERR_ARG, b"codes must be 16-byte"),
        ((P(0x1000), ctypes.byref(m), 9, 8, P(0x2004), None), ERR_ARG, b"image must be 16-byte"),
    ]:
        assert f(*args) == status
        assert word in lib.admmq_last_error(), lib.admmq_last_error()
    g = lib.admmq_packed_taps_i8_bytes
    for ntaps in (1, 3, 9, 25, 49):
        for K, Kp in [(1, 64), (63, 64), (64, 64), (65, 128), (70, 128), (1141, 1152), (65536, 65536)]:
            assert g(ntaps, K) == ntaps * Kp, (ntaps, K)
    for bad in [(0, 8), (50, 8), (-1, 8), (9, 0), (9, -2), (9, 65537)]:
        assert g(*bad) == 0
    from admmq.packed import taps_kp
    assert [taps_kp(K) for K in (1, 63, 64, 65, 1141)] == [64, 64, 64, 128, 1152]


def test_workspace_size_equals_the_integer_gemms(lib):
    f, g = lib.admmq_packed_idwgemm_workspace_size, lib.admmq_packed_igemm_workspace_size
    some = 0
    for M in (1, 64, 65, 128, 512, 2048):
        for K in (1, 64, 65, 130, 286, 1141, 65536):
            for Ho, Wo in ((1, 1), (5, 5), (7, 7), (28, 28), (32, 32), (3, 50)):
                for nb in (1, 3, 4, 64):
                    w = f(M, K, Ho, Wo, nb)
                    assert w == g(M, K, Ho * Wo, nb), (M, K, Ho, Wo, nb)
                    assert w == f(M, K, Ho, Wo, nb)
                    some += w > 0
    assert some > 0
    assert f(512, 1141, 7, 7, 1) == 18 * 512 * 49 * 4      # 18 K pieces of 64: one int32 partial image each
    assert f(256, 130, 32, 32, 4) == 0                     # 256 tiles: the serial regime
    for bad in [(0, 8, 2, 2, 1), (8, 0, 2, 2, 1), (8, 8, 0, 2, 1), (8, 8, 2, -1, 1), (8, 8, 2, 2, 0), (8, 65537, 2, 2, 1),
                (8, 8, 1 << 31, 2, 1), (1 << 40, 8, 2, 2, 1)]:
        assert f(*bad) == 0


def test_meta_kernels_give_shapes_and_dtypes():
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)
    img = ops.packed_taps_i8(torch.empty(9 * 70 // 2, dtype=torch.uint8, device=m), words, 9, 70)
    assert tuple(img.shape) == (9, 128) and img.dtype == torch.int8
    wc = torch.empty(65 * 70 // 2, dtype=torch.uint8, device=m)
    rs = torch.empty(65, dtype=torch.int32, device=m)
    x = torch.empty(3, 70, 7, 6, dtype=torch.uint8, device=m)
    y, mc, c = ops.packed_idwgemm(wc, words, 65, 70, x, 8, -0.7, 2.3, img, 0.125, 3, 3, 2, 2, 1, 1, rs, None, 6, -1.0, 2.0, 0, 0.0,
                                  0.0, False, True)
    assert tuple(y.shape) == (3, 65, 4, 3) and y.dtype == torch.float32
    assert tuple(mc.shape) == (1,) and mc.dtype == torch.int32 and c.numel() == 0
    y, mc, c = ops.packed_idwgemm(wc, words, 65, 70, x, 8, -0.7, 2.3, img, 0.125, 3, 3, 1, 1, 1, 1, rs,
                                  torch.empty(65, device=m), 6, -1.0, 2.0, 5, -1.0, 2.0, True, True)
    assert tuple(y.shape) == (3, 65, 7, 6) and y.dtype == torch.uint8
    assert tuple(mc.shape) == (1,) and tuple(c.shape) == (1,) and c.dtype == torch.int32


def _host_packed(shape, bits=4, scheme="tensor_symmetric", zp=0):
    from admmq import PackedTensor
    from admmq.packed import packed_bytes
    n = shape[0] * shape[1]
    return PackedTensor(codes=torch.zeros(packed_bytes(n, bits), dtype=torch.uint8), shape=tuple(shape), bits=bits,
                        qscheme=scheme, scale=0.25, zero_point=zp, mn=0.0, rng=1.0, index=-1)


def test_python_wrappers_check_their_arguments_on_the_host():
    import admmq
    from admmq import QuantizedActivation
    p, C = _host_packed((6, 10)), _host_packed((9, 10))
    xq = QuantizedActivation(torch.zeros(1, 10, 4, 4, dtype=torch.uint8), 8, -1.0, 2.0)
    mid = (6, -1.0, 1.0)
    f = admmq.packed_depthwise_conv1x1_int
    with pytest.raises(ValueError, match="tensor_minmax"):
        f(xq, C, _host_packed((6, 10), scheme="tensor_minmax"), mid_act=mid)
    with pytest.raises(ValueError, match="tensor_minmax"):
        f(xq, _host_packed((9, 10), scheme="tensor_minmax"), p, mid_act=mid)
    with pytest.raises(ValueError, match="int8"):
        f(xq, _host_packed((9, 10), bits=8, scheme="tensor_affine", zp=3), p, mid_act=mid)
    with pytest.raises(ValueError, match="quantizer"):
        f(xq, C, p)                                         # the mid quantizer is mandatory
    with pytest.raises(ValueError, match="2 <= bits <= 8"):
        f(xq, C, p, mid_act=(9, -1.0, 1.0))
    with pytest.raises(ValueError, match="2 <= bits <= 8"):
        f(QuantizedActivation(xq.codes, 1, -1.0, 2.0), C, p, mid_act=mid)
    with pytest.raises(ValueError, match="out_codes=True needs act"):
        f(xq, C, p, mid_act=mid, out_codes=True)
    with pytest.raises(ValueError, match="2 <= bits <= 8"):
        f(xq, C, p, mid_act=mid, act=(12, -1.0, 1.0), out_codes=True)
    with pytest.raises(TypeError, match="QuantizedActivation"):
        f(torch.zeros(1, 10, 4, 4), C, p, mid_act=mid)
    with pytest.raises(ValueError, match="C must be"):
        f(xq, _host_packed((25, 10)), p, mid_act=mid)
    with pytest.raises(ValueError, match="49"):
        admmq.packed_taps_int(_host_packed((50, 10)))
    with pytest.raises(RuntimeError, match="ROCm GPU"):    # CPU tensors: no CPU implementation
        admmq.packed_taps_int(C)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        f(xq, (torch.zeros(9, 64, dtype=torch.int8), 0.25), p, mid_act=mid)


def test_builder_checks_integer_arguments():
    from admmq import export
    R, cin, cout, ks = 5, 8, 12, (3, 3)
    A, B, C = _host_packed((cout, R)), _host_packed((cin, R)), _host_packed((9, R))
    acts = [(6, -1.0, 1.0), (5, -2.0, 1.0), None]
    in_act = (8, -1.0, 1.0)

    def build(**kw):
        return export.build_cp_layer(R, kw.pop("factors", [A, B, C]), None, cin, cout, ks, 1, 1, **kw)

    with pytest.raises(ValueError, match="in_act"):
        build(act_quant=acts, integer=True)
    with pytest.raises(ValueError, match="conv1 entry"):
        build(act_quant=[None, acts[1], None], integer=True, in_act=in_act)
    with pytest.raises(ValueError, match="conv2 entry"):
        build(act_quant=[acts[0], None, None], integer=True, in_act=in_act)
    with pytest.raises(ValueError, match="conv1 entry"):
        build(integer=True, in_act=in_act)
    with pytest.raises(ValueError, match="PackedTensor"):
        build(factors=[torch.zeros(cout, R), torch.zeros(cin, R), torch.zeros(9, R)], act_quant=acts, integer=True,
              in_act=in_act)
    with pytest.raises(ValueError, match="2 <= bits <= 8"):
        build(act_quant=acts, integer=True, in_act=(1, -1.0, 1.0))
    with pytest.raises(ValueError, match="2 <= bits <= 8"):
        build(act_quant=[(12, -1.0, 1.0), acts[1], None], integer=True, in_act=in_act)
    with pytest.raises(ValueError, match="2 <= bits <= 8"):
        build(act_quant=[acts[0], (9, -1.0, 1.0), None], integer=True, in_act=in_act)
    # factorized_conv hands both words on, for a k x k conv and for a 1x1 conv
    conv = torch.nn.Conv2d(cin, cout, ks, padding=1)
    with pytest.raises(ValueError, match="in_act"):
        export.factorized_conv(conv, R, [A, B, C], act_quant=acts, integer=True)
    with pytest.raises(ValueError, match="in_act"):
        export.factorized_conv(torch.nn.Conv2d(cin, cout, 1), R, [A, B], act_quant=acts[:2], integer=True)
