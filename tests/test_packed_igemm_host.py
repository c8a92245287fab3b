"""Integer packed GEMM, host side (no GPU): every refusal of the new entry points comes back
with its documented status and its own error text before any device call (made-up device
addresses), the workspace query is a function of its arguments, and the Python wrappers and the
2-way builders check their arguments on the host."""
import ctypes

import pytest
import torch

OK, ERR_ARG, ERR_WORKSPACE, ERR_SCHEME = 0, -1, -3, -4
MSE, MINMAX, SYMMETRIC, AFFINE = 0, 1, 2, 3


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


def _call(lib, meta="ok", codes=0x1000, x=0x10001, xq="ok", rs=0x30000, y=0x20000, yc=0, out=None, clamped=0, M=8, K=8,
          N=4, nb=1, x_layout=0, bias=0, ws=0x100000, ws_bytes=1 << 20, trans=0):
    m = _meta() if meta == "ok" else meta
    q = _actq() if xq == "ok" else xq
    return lib.admmq_packed_igemm(ctypes.c_void_p(codes), ctypes.byref(m) if m is not None else None, trans, M, K,
                                  ctypes.c_void_p(x), ctypes.byref(q) if q is not None else None, ctypes.c_void_p(rs),
                                  x_layout, N, nb, ctypes.c_void_p(bias), ctypes.c_void_p(y), ctypes.c_void_p(yc),
                                  ctypes.byref(out) if out is not None else None, ctypes.c_void_p(clamped),
                                  ctypes.c_void_p(ws), ws_bytes, None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(codes=0), ERR_ARG, b"NULL"),
    (dict(x=0), ERR_ARG, b"NULL"),
    (dict(meta=None), ERR_ARG, b"NULL"),
    (dict(rs=0), ERR_ARG, b"NULL"),
    (dict(xq=None), ERR_ARG, b"NULL"),
    (dict(y=0), ERR_ARG, b"exactly one"),
    (dict(yc=0x40000), ERR_ARG, b"exactly one"),
    (dict(M=0), ERR_ARG, b"positive"),
    (dict(K=-3), ERR_ARG, b"positive"),
    (dict(N=0), ERR_ARG, b"positive"),
    (dict(nb=0), ERR_ARG, b"positive"),
    (dict(meta=(MSE, 0)), ERR_ARG, b"bits"),
    (dict(meta=(SYMMETRIC, 9)), ERR_ARG, b"bits"),
    (dict(meta=(4, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(MINMAX, 4)), ERR_SCHEME, b"tensor_minmax"),
    (dict(meta=(AFFINE, 4, 2)), ERR_ARG, b"bad"),
    (dict(meta=(AFFINE, 8, 0, 1)), ERR_ARG, b"int8"),       # -128 - 1 < -128
    (dict(meta=(AFFINE, 8, 0, -1)), ERR_ARG, b"int8"),      # 127 + 1 > 127
    (dict(K=65537), ERR_ARG, b"65536"),
    (dict(xq=(1,)), ERR_ARG, b"2..8"),
    (dict(xq=(9,)), ERR_ARG, b"2..8"),
    (dict(xq=(8, 0)), ERR_ARG, b"x_q"),
    (dict(y=0, yc=0x40001), ERR_ARG, b"codes output"),                 # no out_q
    (dict(y=0, yc=0x40001, out=(9,)), ERR_ARG, b"codes output"),
    (dict(out=(25,)), ERR_ARG, b"1..24"),
    (dict(x_layout=1, nb=2), ERR_ARG, b"nb = 1"),
    (dict(x_layout=2), ERR_ARG, b"x_layout"),
    (dict(trans=2), ERR_ARG, b"trans_w"),
    (dict(codes=0x1004), ERR_ARG, b"16-byte"),
    (dict(y=0x20002), ERR_ARG, b"aligned"),
    (dict(bias=0x50001), ERR_ARG, b"aligned"),
    (dict(rs=0x30002), ERR_ARG, b"aligned"),
    (dict(M=1 << 30), ERR_ARG, b"range"),
    (dict(M=512, K=1141, N=4, ws_bytes=16), ERR_WORKSPACE, b"workspace"),
    (dict(M=512, K=1141, N=4, ws=0, ws_bytes=1 << 30), ERR_WORKSPACE, b"workspace"),
])
def test_packed_igemm_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    for k in ("xq", "out"):
        if isinstance(kw.get(k), tuple):
            kw[k] = _actq(*kw[k])
    assert _call(lib, **kw) == status
    assert word in lib.admmq_last_error(), lib.admmq_last_error()


def test_allowed_affine_records_pass_the_record_check(lib):
    """An affine record whose integers fit int8 gets past the record check (the next refusal is
    the short workspace), so the int8 refusal above is about the range and nothing else."""
    for bits, zp in [(8, 0), (7, 63), (7, -64), (4, -8), (1, 0)]:
        assert _call(lib, meta=_meta(AFFINE, bits, 0, zp), M=512, K=1141, N=4, ws_bytes=16) == ERR_WORKSPACE


def test_rowsums_and_code_entry_refusals(lib):
    P = ctypes.c_void_p
    m = _meta()
    f = lib.admmq_packed_rowsums
    for args, status, word in [
        ((P(0), ctypes.byref(m), 0, 8, 8, P(0x2000), None), ERR_ARG, b"NULL"),
        ((P(0x1000), ctypes.byref(m), 0, 8, 8, P(0), None), ERR_ARG, b"NULL"),
        ((P(0x1000), ctypes.byref(m), 0, 0, 8, P(0x2000), None), ERR_ARG, b"positive"),
        ((P(0x1000), ctypes.byref(_meta(MINMAX, 4)), 0, 8, 8, P(0x2000), None), ERR_SCHEME, b"tensor_minmax"),
        ((P(0x1000), ctypes.byref(_meta(AFFINE, 8, 0, 5)), 0, 8, 8, P(0x2000), None), ERR_ARG, b"int8"),
        ((P(0x1000), ctypes.byref(m), 0, 8, 65537, P(0x2000), None), ERR_ARG, b"65536"),
        ((P(0x1000), ctypes.byref(m), 3, 8, 8, P(0x2000), None), ERR_ARG, b"trans_w"),
        ((P(0x1008), ctypes.byref(m), 0, 8, 8, P(0x2000), None), ERR_ARG, b"16-byte"),
        ((P(0x1000), ctypes.byref(m), 0, 8, 8, P(0x2002), None), ERR_ARG, b"aligned"),
    ]:
        assert f(*args) == status
        assert word in lib.admmq_last_error(), lib.admmq_last_error()
    q = _actq(5)
    enc, dec = lib.admmq_act_encode, lib.admmq_act_decode
    for call, word in [
        (lambda: enc(P(0), P(0x2001), 10, ctypes.byref(q), P(0), None), b"NULL"),
        (lambda: enc(P(0x1000), P(0), 10, ctypes.byref(q), P(0), None), b"NULL"),
        (lambda: enc(P(0x1000), P(0x2001), 10, None, P(0), None), b"q must not"),
        (lambda: enc(P(0x1000), P(0x2001), 10, ctypes.byref(_actq(5, 0)), P(0), None), b"q must not"),
        (lambda: enc(P(0x1000), P(0x2001), 10, ctypes.byref(_actq(1)), P(0), None), b"2..8"),
        (lambda: enc(P(0x1000), P(0x2001), 10, ctypes.byref(_actq(9)), P(0), None), b"2..8"),
        (lambda: enc(P(0x1000), P(0x2001), 0, ctypes.byref(q), P(0), None), b"positive"),
        (lambda: enc(P(0x1002), P(0x2001), 10, ctypes.byref(q), P(0), None), b"float aligned"),
        (lambda: enc(P(0x1000), P(0x2001), 10, ctypes.byref(q), P(0x3001), None), b"int32 aligned"),
        (lambda: dec(P(0), P(0x2000), 10, ctypes.byref(q), None), b"NULL"),
        (lambda: dec(P(0x1001), P(0), 10, ctypes.byref(q), None), b"NULL"),
        (lambda: dec(P(0x1001), P(0x2000), 10, None, None), b"q must not"),
        (lambda: dec(P(0x1001), P(0x2000), 10, ctypes.byref(_actq(1)), None), b"2..8"),
        (lambda: dec(P(0x1001), P(0x2000), -1, ctypes.byref(q), None), b"positive"),
        (lambda: dec(P(0x1001), P(0x2002), 10, ctypes.byref(q), None), b"float aligned"),
    ]:
        assert call() == ERR_ARG
        assert word in lib.admmq_last_error(), lib.admmq_last_error()


def test_workspace_size_is_a_function_of_its_arguments(lib):
    f = lib.admmq_packed_igemm_workspace_size
    for bad in [(0, 8, 8, 1), (8, 0, 8, 1), (8, 8, -1, 1), (8, 8, 8, 0), (1 << 40, 8, 8, 1), (8, 65537, 8, 1)]:
        assert f(*bad) == 0
    shapes = [(512, 1141, 4, 1), (1141, 512, 49, 1), (64, 134, 49, 3), (4096, 1024, 1, 1), (4096, 1024, 512, 1),
              (134, 64, 65, 2), (64, 65536, 1, 1)]
    first = [f(*s) for s in shapes]
    assert [f(*s) for s in shapes] == first
    # few output tiles: the K pieces run as separate workgroups and need their int32 partial images
    assert first[0] > 0 and first[0] % (512 * 4 * 4) == 0
    # one K piece (K <= 64) or at least 256 tiles: nothing
    assert first[5] == 0 and first[4] == 0
    for s, b in zip(shapes, first):
        assert b % (s[0] * s[2] * s[3] * 4) == 0


def _host_packed(shape, bits=4, scheme="tensor_symmetric", zp=0):
    from admmq import PackedTensor
    from admmq.packed import packed_bytes
    n = shape[0] * shape[1]
    return PackedTensor(codes=torch.zeros(packed_bytes(n, bits), dtype=torch.uint8), shape=tuple(shape), bits=bits,
                        qscheme=scheme, scale=0.25, zero_point=zp, mn=0.0, rng=1.0, index=-1)


def test_python_wrappers_check_their_arguments_on_the_host():
    import admmq
    from admmq import QuantizedActivation
    p = _host_packed((6, 10))
    xq = QuantizedActivation(torch.zeros(3, 10, dtype=torch.uint8), 8, -1.0, 2.0)
    with pytest.raises(ValueError, match="tensor_minmax"):
        admmq.packed_linear_int(xq, _host_packed((6, 10), scheme="tensor_minmax"))
    with pytest.raises(ValueError, match="int8"):
        admmq.packed_linear_int(xq, _host_packed((6, 10), bits=8, scheme="tensor_affine", zp=3))
    with pytest.raises(ValueError, match="65536"):
        admmq.packed_linear_int(xq, _host_packed((2, 65537)))
    with pytest.raises(ValueError, match="out_codes=True needs act"):
        admmq.packed_linear_int(xq, p, out_codes=True)
    with pytest.raises(ValueError, match="out_codes=True needs act"):
        admmq.packed_conv1x1_int(QuantizedActivation(torch.zeros(1, 10, 2, 2, dtype=torch.uint8), 8, -1.0, 2.0), p,
                                 out_codes=True)
    with pytest.raises(ValueError, match="2 <= bits <= 8"):
        admmq.packed_linear_int(xq, p, act=(9, -1.0, 1.0), out_codes=True)
    with pytest.raises(ValueError, match="2 <= bits <= 8"):
        admmq.packed_linear_int(QuantizedActivation(xq.codes, 1, -1.0, 2.0), p)
    with pytest.raises(TypeError, match="QuantizedActivation"):
        admmq.packed_linear_int(torch.zeros(3, 10), p)
    with pytest.raises(ValueError, match="H, W"):
        admmq.packed_conv1x1_int(xq, p)
    with pytest.raises(ValueError, match="2 <= bits <= 8"):
        admmq.act_encode(torch.zeros(4), (1, -1.0, 1.0))
    with pytest.raises(ValueError, match="quantizer"):
        admmq.act_encode(torch.zeros(4), None)
    # CPU tensors: no CPU implementation
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.act_encode(torch.zeros(4), (8, -1.0, 1.0))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.act_decode(torch.zeros(4, dtype=torch.uint8), 8, -1.0, 2.0)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_rowsums(p)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        xq.dequantize()


def test_builders_check_integer_arguments():
    from admmq import export
    R, cin, cout = 5, 8, 12
    A, B = _host_packed((cout, R)), _host_packed((cin, R))
    acts = [(6, -1.0, 1.0), None]
    for build in (lambda **kw: export.build_cp2conv_layer(R, kw.pop("factors", [A, B]), None, cin, cout, 0, 1, **kw),
                  lambda **kw: export.build_cpfc_layer(R, kw.pop("factors", [A, B]), None, cin, cout, **kw)):
        with pytest.raises(ValueError, match="in_act"):
            build(act_quant=acts, integer=True)
        with pytest.raises(ValueError, match="inter-stage"):
            build(act_quant=[None, (8, -1.0, 1.0)], integer=True, in_act=(8, -1.0, 1.0))
        with pytest.raises(ValueError, match="inter-stage"):
            build(integer=True, in_act=(8, -1.0, 1.0))
        with pytest.raises(ValueError, match="PackedTensor"):
            build(factors=[torch.zeros(cout, R), torch.zeros(cin, R)], act_quant=acts, integer=True, in_act=(8, -1.0, 1.0))
        with pytest.raises(ValueError, match="2 <= bits <= 8"):
            build(act_quant=acts, integer=True, in_act=(1, -1.0, 1.0))
        with pytest.raises(ValueError, match="2 <= bits <= 8"):
            build(act_quant=[(12, -1.0, 1.0), None], integer=True, in_act=(8, -1.0, 1.0))
        with pytest.raises(ValueError, match="tensor_minmax"):
            build(factors=[_host_packed((cout, R), scheme="tensor_minmax"), B], act_quant=acts, integer=True,
                  in_act=(8, -1.0, 1.0))
        # on the host the layer builds (its forward needs the GPU); the defaults build today's module
        layer = build(act_quant=acts, integer=True, in_act=(8, -1.0, 1.0))
        assert type(layer) is export.IntegerPackedPair
        names = [n for n, _ in layer.named_children()]
        assert names in (["conv1", "conv2"], ["fc1", "fc2"])
        first, last = (getattr(layer, n) for n in names)
        assert first.transpose and not last.transpose and first._act == (6, -1.0, 2.0) and last._act is None
        sd = layer.state_dict()
        assert sd["_extra_state"]["in_act"] == [8, -1.0, 2.0] and sd["_extra_state"]["rowsums"] == [None, None]
        assert type(build()) is torch.nn.Sequential
        assert type(build(act_quant=acts)) is torch.nn.Sequential
