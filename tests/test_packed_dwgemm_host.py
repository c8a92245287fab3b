"""Fused depthwise + 1x1 stage, host side (no GPU): every refusal of admmq_packed_dwgemm comes
back with its documented status and text before any device call (made-up device addresses), the
workspace query equals admmq_packed_gemm's for (M, K, Ho Wo, nb), the Meta kernel propagates
shapes, CPU tensors raise, and build_cp_layer(fused=True) refuses float factors and a
mis-shaped C."""
import ctypes

import pytest
import torch

OK, ERR_ARG, ERR_WORKSPACE = 0, -1, -3
MSE, MINMAX, SYMMETRIC, AFFINE = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    return _lib.load()


def _meta(scheme=MSE, bits=4, bad=0):
    from admmq import _lib
    return _lib.QMeta(scheme, bits, 0.125, 0, 0.0, 1.0, -1, bad)


def _call(lib, meta="ok", codes=0x1000, t=0x10000, taps=0x18000, y=0x20000, M=8, K=8, nb=1, H=6, W=6, kh=3, kw=3, sh=1,
          sw=1, ph=1, pw=1, bias=0, ws=0x100000, ws_bytes=1 << 20):
    m = _meta() if meta == "ok" else meta
    return lib.admmq_packed_dwgemm(ctypes.c_void_p(codes), ctypes.byref(m) if m is not None else None, M, K,
                                   ctypes.c_void_p(t), nb, H, W, ctypes.c_void_p(taps), kh, kw, sh, sw, ph, pw,
                                   ctypes.c_void_p(bias), ctypes.c_void_p(y), ctypes.c_void_p(ws), ws_bytes, None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(codes=0), ERR_ARG, b"NULL"),
    (dict(t=0), ERR_ARG, b"NULL"),
    (dict(taps=0), ERR_ARG, b"NULL"),
    (dict(y=0), ERR_ARG, b"NULL"),
    (dict(meta=None), ERR_ARG, b"NULL"),
    (dict(M=0), ERR_ARG, b"positive"),
    (dict(K=-3), ERR_ARG, b"positive"),
    (dict(H=0), ERR_ARG, b"positive"),
    (dict(W=-1), ERR_ARG, b"positive"),
    (dict(nb=0), ERR_ARG, b"positive"),
    (dict(meta=(MSE, 0)), ERR_ARG, b"bits"),
    (dict(meta=(SYMMETRIC, 9)), ERR_ARG, b"bits"),
    (dict(meta=(4, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(-1, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(MINMAX, 1)), ERR_ARG, b"1 bit"),
    (dict(meta=(AFFINE, 4, 2)), ERR_ARG, b"bad"),
    (dict(kh=0), ERR_ARG, b"kernel size"),
    (dict(kw=8, pw=1), ERR_ARG, b"kernel size"),
    (dict(sh=0), ERR_ARG, b"stride"),
    (dict(sw=-2), ERR_ARG, b"stride"),
    (dict(ph=3), ERR_ARG, b"padding"),
    (dict(pw=-1), ERR_ARG, b"padding"),
    (dict(kh=1, ph=1), ERR_ARG, b"padding"),
    (dict(H=2, kh=5, ph=1), ERR_ARG, b"does not fit"),
    (dict(W=1, kw=3, pw=0), ERR_ARG, b"does not fit"),
    (dict(codes=0x1004), ERR_ARG, b"16-byte"),
    (dict(t=0x10002), ERR_ARG, b"float aligned"),
    (dict(taps=0x18001), ERR_ARG, b"float aligned"),
    (dict(y=0x20002), ERR_ARG, b"float aligned"),
    (dict(bias=0x30003), ERR_ARG, b"float aligned"),
    (dict(M=1 << 30), ERR_ARG, b"range"),
    (dict(H=1 << 41), ERR_ARG, b"range"),
    (dict(K=1 << 20, H=1 << 10, W=1 << 10), ERR_ARG, b"2^40"),
    (dict(nb=1 << 10, K=1 << 10, H=1 << 10, W=1 << 10, sh=64, sw=64), ERR_ARG, b"2^40"),
    (dict(M=512, K=1141, H=2, W=2, ws_bytes=16), ERR_WORKSPACE, b"workspace"),
    (dict(M=512, K=1141, H=2, W=2, ws=0, ws_bytes=1 << 30), ERR_WORKSPACE, b"workspace"),
    (dict(M=512, K=1141, H=2, W=2, ws=0x100002), ERR_ARG, b"workspace must be float aligned"),
])
def test_packed_dwgemm_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    assert _call(lib, **kw) == status
    assert word in lib.admmq_last_error()


def test_every_refusal_has_its_own_text(lib):
    """One call per class of refusal: the texts differ pairwise."""
    calls = [dict(codes=0), dict(M=0), dict(meta=_meta(MSE, 0)), dict(meta=_meta(4, 4)), dict(meta=_meta(MINMAX, 1)),
             dict(meta=_meta(AFFINE, 4, 2)), dict(kh=0), dict(sh=0), dict(ph=3), dict(H=2, kh=5, ph=1),
             dict(codes=0x1004), dict(t=0x10002), dict(M=1 << 30), dict(K=1 << 20, H=1 << 10, W=1 << 10),
             dict(M=512, K=1141, H=2, W=2, ws_bytes=16), dict(M=512, K=1141, H=2, W=2, ws=0x100002)]
    texts = []
    for kw in calls:
        assert _call(lib, **kw) != OK
        texts.append(lib.admmq_last_error())
    assert len(set(texts)) == len(texts), texts


def test_workspace_size_equals_the_gemms(lib):
    f, g = lib.admmq_packed_dwgemm_workspace_size, lib.admmq_packed_gemm_workspace_size
    shapes = [(512, 1141, 7, 7, 1), (512, 1141, 7, 7, 64), (128, 286, 28, 28, 1), (64, 134, 7, 7, 3), (33, 65, 4, 4, 2),
              (128, 1141, 2, 2, 1), (134, 134, 31, 31, 6), (64, 40, 4, 4, 1), (40, 70, 5, 5, 1), (4096, 1024, 1, 1, 1)]
    sizes = [f(*s) for s in shapes]
    assert sizes == [g(M, K, Ho * Wo, nb) for M, K, Ho, Wo, nb in shapes]
    assert sizes == [f(*s) for s in shapes]
    assert sizes[0] > 0 and sizes[5] > 0       # few tiles, several K pieces: the partial images
    assert sizes[1] == 0 and sizes[6] == 0     # many tiles: serial
    assert sizes[7] == 0                       # one K piece
    for bad in [(0, 8, 4, 4, 1), (8, 0, 4, 4, 1), (8, 8, 0, 4, 1), (8, 8, 4, -1, 1), (8, 8, 4, 4, 0), (1 << 40, 8, 4, 4, 1),
                (8, 1 << 40, 4, 4, 1), (8, 8, 1 << 31, 4, 1), (8, 8, 1 << 20, 1 << 20, 1), (8, 8, 1 << 62, 1 << 62, 1)]:
        assert f(*bad) == 0, bad


def test_meta_kernel_gives_the_shapes():
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=m)
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)

    def shape(x, k, s, p, taps=None, bias=None):
        taps = torch.empty(k[0] * k[1], 134, device=m) if taps is None else taps
        y = ops.packed_dwgemm(codes, words, 64, 134, torch.empty(*x, device=m), taps, k[0], k[1], s[0], s[1], p[0], p[1],
                              bias)
        assert y.dtype == torch.float32 and y.device.type == "meta"
        return tuple(y.shape)

    assert shape((3, 134, 7, 7), (3, 3), (1, 1), (1, 1)) == (3, 64, 7, 7)
    assert shape((2, 134, 7, 7), (3, 3), (2, 2), (1, 1)) == (2, 64, 4, 4)        # odd H, stride 2
    assert shape((2, 134, 8, 8), (3, 3), (2, 2), (1, 1)) == (2, 64, 4, 4)
    assert shape((1, 134, 5, 9), (1, 3), (1, 2), (0, 1)) == (1, 64, 5, 5)
    assert shape((1, 134, 9, 9), (5, 5), (1, 1), (2, 2), bias=torch.empty(64, device=m)) == (1, 64, 9, 9)
    assert shape((1, 134, 6, 6), (3, 3), (1, 1), (0, 0)) == (1, 64, 4, 4)
    assert shape((1, 134, 7, 6), (3, 2), (3, 2), (0, 1)) == (1, 64, 2, 4)
    with pytest.raises(RuntimeError, match="x must be"):
        shape((3, 64, 7, 7), (3, 3), (1, 1), (1, 1))
    with pytest.raises(RuntimeError, match="taps must be"):
        shape((3, 134, 7, 7), (3, 3), (1, 1), (1, 1), taps=torch.empty(134, 9, device=m))
    with pytest.raises(RuntimeError, match="kernel size"):
        shape((3, 134, 9, 9), (8, 1), (1, 1), (0, 0))
    with pytest.raises(RuntimeError, match="padding"):
        shape((3, 134, 7, 7), (3, 3), (1, 1), (3, 1))
    with pytest.raises(RuntimeError, match="stride"):
        shape((3, 134, 7, 7), (3, 3), (0, 1), (1, 1))
    with pytest.raises(RuntimeError, match="does not fit"):
        shape((3, 134, 2, 7), (5, 3), (1, 1), (1, 1))


def _host_packed(shape, bits=4):
    from admmq import PackedTensor
    from admmq.packed import packed_bytes
    n = shape[0] * shape[1]
    return PackedTensor(codes=torch.zeros(packed_bytes(n, bits), dtype=torch.uint8), shape=tuple(shape), bits=bits,
                        qscheme="tensor_symmetric", scale=0.25, zero_point=0, mn=0.0, rng=0.0, index=-1)


def test_cpu_tensors_raise():
    import admmq
    from admmq import _lib, export
    p = _host_packed((6, 10))
    x, taps = torch.zeros(2, 10, 5, 5), torch.zeros(9, 10)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_depthwise_conv1x1(x, taps, p, kernel_size=(3, 3), padding=1)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        export.PackedDepthwiseConv1x1(p, taps, torch.zeros(6), (3, 3), 1, 1)(x)
    with pytest.raises((RuntimeError, NotImplementedError)):   # no CPU kernel: the dispatcher or the op refuses
        _lib.ops().packed_dwgemm(p.codes, torch.tensor([2, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32), 6, 10, x, taps, 3, 3,
                                 1, 1, 1, 1, None)
    with pytest.raises(ValueError, match="2-D"):
        admmq.packed_depthwise_conv1x1(x, taps, admmq.PackedTensor(codes=p.codes, shape=(6, 5, 2), bits=4,
                                                                   qscheme="tensor_symmetric", scale=0.25, zero_point=0,
                                                                   mn=0.0, rng=0.0, index=-1))


def test_the_module_holds_codes_taps_and_geometry():
    from admmq import export
    p = _host_packed((6, 10), bits=3)
    taps = torch.arange(90, dtype=torch.float32).reshape(9, 10)
    m = export.PackedDepthwiseConv1x1(p, taps, torch.ones(6), (3, 3), 2, 1)
    assert isinstance(m, export._PackedWeight) and not hasattr(m, "weight") and not m.transpose
    assert (m.in_features, m.out_features) == (10, 6)
    assert (m.kernel_size, m.stride, m.padding) == ((3, 3), (2, 2), (1, 1))
    assert m.taps.dtype == torch.float32 and torch.equal(m.taps, taps) and m.taps.data_ptr() != taps.data_ptr()
    sd = m.state_dict()
    assert set(sd) == {"codes", "taps", "bias", "_extra_state"}
    es = sd["_extra_state"]
    assert es["kernel_size"] == [3, 3] and es["stride"] == [2, 2] and es["padding"] == [1, 1] and es["bits"] == 3
    other = export.PackedDepthwiseConv1x1(_host_packed((6, 10), bits=3), torch.zeros(9, 10), torch.zeros(6), (3, 3), 1, 0)
    other.load_state_dict(sd)
    assert torch.equal(other.taps, taps) and (other.stride, other.padding) == ((2, 2), (1, 1))
    assert bool((other.bias == 1).all())
    with pytest.raises(AssertionError, match="Expected shape"):
        export.PackedDepthwiseConv1x1(p, torch.zeros(10, 9), None, (3, 3))
    with pytest.raises(AssertionError, match="Expected shape"):
        export.PackedDepthwiseConv1x1(p, torch.zeros(9, 10), torch.zeros(7), (3, 3))
    with pytest.raises(TypeError, match="float32"):
        export.PackedDepthwiseConv1x1(p, torch.zeros(9, 10, dtype=torch.float64), None, (3, 3))
    wrong = export.PackedDepthwiseConv1x1(_host_packed((6, 10), bits=3), torch.zeros(9, 10), torch.zeros(6), (1, 9))
    with pytest.raises((ValueError, RuntimeError)):
        wrong.load_state_dict(sd)


def test_fused_builders_refuse_float_factors_and_a_misshaped_C():
    from admmq import export
    R, cin, cout = 5, 8, 12
    A, B, C = _host_packed((cout, R)), _host_packed((cin, R)), _host_packed((9, R))
    fl = [torch.zeros(cout, R), torch.zeros(cin, R), torch.zeros(9, R)]
    with pytest.raises(ValueError, match="PackedTensor"):
        export.build_cp_layer(R, fl, None, cin, cout, (3, 3), 1, 1, fused=True)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1)
    with pytest.raises(ValueError, match="PackedTensor"):
        export.factorized_conv(conv, R, fl, fused=True)
    with pytest.raises(AssertionError, match=r"Expected shape: \(9, 5\), but got \(4, 5\)"):
        export.build_cp_layer(R, [A, B, _host_packed((4, R))], None, cin, cout, (3, 3), 1, 1, fused=True)
    with pytest.raises(AssertionError, match=r"Expected shape: \(9, 5\), but got \(9, 6\)"):
        export.factorized_conv(conv, R, [A, B, _host_packed((9, 6))], fused=True)
    with pytest.raises(AssertionError, match=r"Expected shape: \(5, 8, 1, 1\), but got \(5, 7, 1, 1\)"):
        export.build_cp_layer(R, [A, _host_packed((7, R)), C], None, cin, cout, (3, 3), 1, 1, fused=True)
    with pytest.raises(NotImplementedError, match="groups"):
        export.build_cp_layer(R, [A, B, C], None, cin, cout, (3, 3), 1, 1, groups=2, fused=True)
    with pytest.raises(ValueError, match="1x1"):
        export.factorized_conv(torch.nn.Conv2d(cin, cout, 1), R, [A, B], fused=True)
    # the default is unchanged: the reference's conv1 / conv2 / conv3 layout on float factors
    seq = export.build_cp_layer(R, fl, None, cin, cout, (3, 3), 1, 1)
    assert [n for n, _ in seq.named_children()] == ["conv1", "conv2", "conv3"]


def test_the_library_exports_both_symbols(lib):
    import admmq
    for name in ("admmq_packed_dwgemm", "admmq_packed_dwgemm_workspace_size"):
        assert getattr(lib, name) is not None
    raw = ctypes.CDLL(lib._name)
    assert raw.admmq_packed_dwgemm and raw.admmq_packed_dwgemm_workspace_size
    assert callable(admmq.packed_depthwise_conv1x1)
