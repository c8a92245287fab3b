"""Packed-weight GEMM, host side (no GPU): every refusal of admmq_packed_gemm comes back with
its documented status before any device call (made-up device addresses), the workspace query
is a function of its arguments, the Meta kernel propagates shapes, CPU tensors raise, and the
export builders refuse mis-shaped PackedTensor factors."""
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


def _call(lib, meta="ok", codes=0x1000, x=0x10000, y=0x20000, M=8, K=8, N=4, nb=1, x_layout=0, bias=0, ws=0x100000,
          ws_bytes=1 << 20, trans=0):
    m = _meta() if meta == "ok" else meta
    return lib.admmq_packed_gemm(ctypes.c_void_p(codes), ctypes.byref(m) if m is not None else None, trans, M, K,
                                 ctypes.c_void_p(x), x_layout, N, nb, ctypes.c_void_p(bias), ctypes.c_void_p(y),
                                 ctypes.c_void_p(ws), ws_bytes, None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(codes=0), ERR_ARG, b"NULL"),
    (dict(x=0), ERR_ARG, b"NULL"),
    (dict(y=0), ERR_ARG, b"NULL"),
    (dict(meta=None), ERR_ARG, b"NULL"),
    (dict(M=0), ERR_ARG, b"positive"),
    (dict(K=-3), ERR_ARG, b"positive"),
    (dict(N=0), ERR_ARG, b"positive"),
    (dict(nb=0), ERR_ARG, b"positive"),
    (dict(meta=(MSE, 0)), ERR_ARG, b"bits"),
    (dict(meta=(SYMMETRIC, 9)), ERR_ARG, b"bits"),
    (dict(meta=(4, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(-1, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(MINMAX, 1)), ERR_ARG, b"1 bit"),
    (dict(meta=(AFFINE, 4, 2)), ERR_ARG, b"bad"),
    (dict(x_layout=1, nb=2), ERR_ARG, b"nb = 1"),
    (dict(x_layout=2), ERR_ARG, b"x_layout"),
    (dict(codes=0x1004), ERR_ARG, b"16-byte"),
    (dict(x=0x10002), ERR_ARG, b"float aligned"),
    (dict(M=1 << 30), ERR_ARG, b"range"),
    (dict(M=512, K=1141, N=4, ws_bytes=16), ERR_WORKSPACE, b"workspace"),
    (dict(M=512, K=1141, N=4, ws=0, ws_bytes=1 << 30), ERR_WORKSPACE, b"workspace"),
])
def test_packed_gemm_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    assert _call(lib, **kw) == status
    assert word in lib.admmq_last_error()


def test_workspace_size_is_a_function_of_its_arguments(lib):
    f = lib.admmq_packed_gemm_workspace_size
    for bad in [(0, 8, 8, 1), (8, 0, 8, 1), (8, 8, -1, 1), (8, 8, 8, 0), (1 << 40, 8, 8, 1), (8, 1 << 40, 8, 1)]:
        assert f(*bad) == 0
    shapes = [(512, 1141, 4, 1), (1141, 512, 49, 1), (64, 134, 49, 3), (4096, 1024, 1, 1), (4096, 1024, 512, 1),
              (134, 64, 65, 2)]
    first = [f(*s) for s in shapes]
    assert [f(*s) for s in shapes] == first
    # few output tiles: the K pieces run as separate workgroups and need their partial images
    assert first[0] > 0 and first[0] % (512 * 4 * 4) == 0
    # one K piece (K <= 64) or many tiles: nothing
    assert first[5] == 0 and first[4] == 0
    # every size is a whole number of output images
    for s, b in zip(shapes, first):
        assert b % (s[0] * s[2] * s[3] * 4) == 0


def _ws_formula(M, K, N, nb, integer):
    """The documented plan, written out: K pieces of kp = max(64, BK ceil(K / (32 BK))) (BK = 32 float, 64 integer);
    the pieces run in parallel, one 4-byte partial image of C M elements each, when there is more than one piece
    and fewer than 256 tiles of 64 x 64; sizes out of range give 0."""
    if min(M, K, N, nb) <= 0 or M > 1 << 22 or N > 1 << 30 or nb > 1 << 30 or nb * N > 1 << 30:
        return 0
    if K > (65536 if integer else 1 << 24) or (not integer and M * K >= 1 << 40):
        return 0
    bk = 64 if integer else 32
    kp = max(64, bk * -(-K // (32 * bk)))
    pieces = -(-K // kp)
    tiles = -(-M // 64) * -(-(nb * N) // 64)
    return pieces * (nb * N * M) * 4 if pieces > 1 and tiles < 256 else 0


def test_workspace_sizes_match_the_closed_formula(lib):
    ks = [1, 63, 64, 65, 2048, 2049, 65536, 65537]
    # (M, N, nb): one tile; partial tiles; 255 and 256 tiles along m and along c; as a product 15 x 17 = 255,
    # 15 x 18, 16 x 16 = 256 and 5 x 51 = 255; a batch
    mnb = [(8, 4, 1), (65, 129, 1), (64 * 255, 64, 1), (64 * 255 + 1, 64, 1), (64, 64 * 255, 1), (64, 64 * 255 + 1, 1),
           (960, 1088, 1), (960, 1089, 1), (1024, 1024, 1), (320, 3264, 1), (134, 65, 3), (512, 7, 2)]
    grid = [(M, K, N, nb) for K in ks for (M, N, nb) in mnb]
    # just inside and just beyond each limit
    grid += [(1 << 22, 65, 1, 1), ((1 << 22) + 1, 65, 1, 1), (8, 1 << 24, 4, 1), (8, (1 << 24) + 1, 4, 1),
             (8, 128, 1 << 30, 1), (8, 128, (1 << 30) + 1, 1), (8, 128, 1, 1 << 30), (8, 128, 1, (1 << 30) + 1),
             (8, 128, 1 << 20, 1 << 10), (8, 128, 1 << 20, (1 << 10) + 1), (1 << 22, (1 << 18) - 1, 1, 1),
             (1 << 22, 1 << 18, 1, 1), (0, 8, 8, 1), (8, 0, 8, 1), (8, 8, 0, 1), (8, 8, 8, 0), (8, 8, -1, 1)]
    for M, K, N, nb in grid:
        assert lib.admmq_packed_gemm_workspace_size(M, K, N, nb) == _ws_formula(M, K, N, nb, False), (M, K, N, nb)
        assert lib.admmq_packed_igemm_workspace_size(M, K, N, nb) == _ws_formula(M, K, N, nb, True), (M, K, N, nb)
        # the depthwise entry points: N = Ho Wo, in both factorisations
        for Ho, Wo in ((N, 1), (1, N)) + (((N // 17, 17),) if N % 17 == 0 else ()):
            for f, integer in ((lib.admmq_packed_dwgemm_workspace_size, False), (lib.admmq_packed_idwgemm_workspace_size, True)):
                assert f(M, K, Ho, Wo, nb) == _ws_formula(M, K, Ho * Wo, nb, integer), (M, K, Ho, Wo, nb, integer)
    # Ho and Wo each at most 2^30 and positive, and their product within N's limit
    for Ho, Wo in [((1 << 30) + 1, 1), (1, (1 << 30) + 1), (1 << 16, 1 << 15), (0, 4), (4, -1)]:
        assert lib.admmq_packed_dwgemm_workspace_size(512, 1141, Ho, Wo, 1) == 0
        assert lib.admmq_packed_idwgemm_workspace_size(512, 1141, Ho, Wo, 1) == 0
    # the parallel regime is in the grid: (8, 65, 4, 1) has two pieces and one tile
    assert lib.admmq_packed_gemm_workspace_size(8, 65, 4, 1) == 2 * 4 * 8 * 4
    assert lib.admmq_packed_idwgemm_workspace_size(64 * 255, 65, 8, 8, 1) == 2 * 64 * (64 * 255) * 4


def test_meta_kernel_gives_the_shapes():
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=m)
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)
    y = ops.packed_gemm(codes, words, False, 64, 134, torch.empty(3, 134, 7, 5, device=m), 0, None)
    assert tuple(y.shape) == (3, 64, 7, 5) and y.dtype == torch.float32
    y = ops.packed_gemm(codes, words, True, 134, 64, torch.empty(3, 64, 7, 5, device=m), 0, None)
    assert tuple(y.shape) == (3, 134, 7, 5)
    y = ops.packed_gemm(codes, words, False, 64, 134, torch.empty(2, 5, 134, device=m), 1, None)
    assert tuple(y.shape) == (2, 5, 64)
    y = ops.packed_gemm(codes, words, True, 134, 64, torch.empty(64, device=m), 1, torch.empty(134, device=m))
    assert tuple(y.shape) == (134,)
    with pytest.raises(RuntimeError, match="x must be"):
        ops.packed_gemm(codes, words, False, 64, 134, torch.empty(3, 64, 7, 5, device=m), 0, None)


def _host_packed(shape, bits=4):
    from admmq import PackedTensor
    from admmq.packed import packed_bytes
    n = shape[0] * shape[1]
    return PackedTensor(codes=torch.zeros(packed_bytes(n, bits), dtype=torch.uint8), shape=tuple(shape), bits=bits,
                        qscheme="tensor_symmetric", scale=0.25, zero_point=0, mn=0.0, rng=0.0, index=-1)


def test_cpu_tensors_raise():
    import admmq
    from admmq import export
    p = _host_packed((6, 10))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_linear(torch.zeros(3, 10), p)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_linear(torch.zeros(3, 6), p, transpose=True)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_conv1x1(torch.zeros(2, 10, 4, 4), p, stride=2)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        export.PackedLinear(p)(torch.zeros(3, 10))
    with pytest.raises(ValueError, match="2-D"):
        admmq.packed_linear(torch.zeros(3, 10),
                            admmq.PackedTensor(codes=p.codes, shape=(6, 5, 2), bits=4, qscheme="tensor_symmetric",
                                               scale=0.25, zero_point=0, mn=0.0, rng=0.0, index=-1))
    bad = _host_packed((6, 10))
    bad.bad = 2
    with pytest.raises(ValueError, match="bad"):
        admmq.packed_linear(torch.zeros(3, 10), bad)


def test_packed_modules_hold_codes_and_no_weight():
    from admmq import export
    p = _host_packed((6, 10), bits=3)
    lin = export.PackedLinear(p, bias=torch.ones(6))
    assert not hasattr(lin, "weight")
    assert (lin.in_features, lin.out_features) == (10, 6)
    assert lin.codes.dtype == torch.uint8 and lin.codes.numel() == p.nbytes
    assert lin.bias is not None and not lin.bias.requires_grad
    t = export.PackedConv1x1(p, transpose=True, stride=2)
    assert (t.in_features, t.out_features) == (6, 10) and t.bias is None and not hasattr(t, "weight")
    sd = lin.state_dict()
    assert set(sd) == {"codes", "bias", "_extra_state"}
    assert sd["_extra_state"]["bits"] == 3 and sd["_extra_state"]["shape"] == [6, 10]
    with pytest.raises(AssertionError, match="Expected shape"):
        export.PackedLinear(p, bias=torch.ones(7))
    other = export.PackedLinear(_host_packed((10, 6), bits=3))
    with pytest.raises((ValueError, RuntimeError)):
        other.load_state_dict(sd)


def test_builders_refuse_misshaped_packed_factors():
    from admmq import export
    R, cin, cout = 5, 8, 12
    A, B, C = _host_packed((cout, R)), _host_packed((cin, R)), _host_packed((9, R))
    msg = r"Expected shape: \(5, 8, 1, 1\), but got \(5, 7, 1, 1\)"
    with pytest.raises(AssertionError, match=msg):
        export.build_cp_layer(R, [A, _host_packed((7, R)), C], None, cin, cout, (3, 3), 1, 1)
    with pytest.raises(AssertionError, match=msg):
        export.build_cp2conv_layer(R, [A, _host_packed((7, R))], None, cin, cout, 0, 1)
    with pytest.raises(AssertionError, match=r"Expected shape: \(12, 5, 1, 1\), but got \(11, 5, 1, 1\)"):
        export.build_cp2conv_layer(R, [_host_packed((11, R)), B], None, cin, cout, 0, 1)
    with pytest.raises(AssertionError, match="Expected shape"):
        export.build_cp_layer(R, [A, B, _host_packed((4, R))], None, cin, cout, (3, 3), 1, 1)
    with pytest.raises(AssertionError, match=r"Expected shape: \(5, 8\), but got \(5, 9\)"):
        export.build_cpfc_layer(R, [_host_packed((cout, R)), _host_packed((9, R))], None, cin, cout)
    with pytest.raises(AssertionError, match=r"Expected shape: \(12,\), but got \(3,\)"):
        export.build_cp2conv_layer(R, [A, B], torch.zeros(3), cin, cout, 0, 1)
    # well-shaped factors on the host: the 1x1 stages build (their forward needs the GPU)
    seq = export.build_cp2conv_layer(R, [A, B], torch.zeros(cout), cin, cout, 0, 2)
    assert [n for n, _ in seq.named_children()] == ["conv1", "conv2"]
    assert isinstance(seq.conv1, export.PackedConv1x1) and seq.conv1.transpose and seq.conv1.stride == (2, 2)
    assert isinstance(seq.conv2, export.PackedConv1x1) and not seq.conv2.transpose
    fc = export.build_cpfc_layer(R, [_host_packed((cout, R)), _host_packed((cin, R))], None, cin, cout)
    assert [n for n, _ in fc.named_children()] == ["fc1", "fc2"] and isinstance(fc.fc1, export.PackedLinear)
    assert fc.fc1.transpose and (fc.fc1.in_features, fc.fc1.out_features) == (cin, R)
