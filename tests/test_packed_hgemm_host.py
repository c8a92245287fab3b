"""Half-precision packed GEMM, host side (no GPU): every refusal of
admmq_packed_hgemm comes back with its status and its own text before any device call (made-up
device addresses), the workspace query matches its written formula, the header declares what the
library exports, the Meta kernel propagates shape and dtype, CPU tensors raise, act= with a half x
and other dtypes are refused as documented, and the packed modules survive .half()."""
import ctypes
import os
import re

import pytest
import torch

OK, ERR_ARG, ERR_WORKSPACE = 0, -1, -3
MSE, MINMAX, SYMMETRIC, AFFINE = 0, 1, 2, 3
DT_F32, DT_F16, DT_BF16 = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    return _lib.load()


def _meta(scheme=MSE, bits=4, bad=0, zp=0):
    from admmq import _lib
    return _lib.QMeta(scheme, bits, 0.125, zp, 0.0, 1.0, -1, bad)


def _call(lib, meta="ok", codes=0x1000, x=0x10000, y=0x20000, M=8, K=8, N=4, nb=1, x_layout=0, bias=0, ws=0x100000,
          ws_bytes=1 << 20, trans=0, xdt=DT_BF16, ydt=DT_BF16):
    m = _meta() if meta == "ok" else meta
    return lib.admmq_packed_hgemm(ctypes.c_void_p(codes), ctypes.byref(m) if m is not None else None, trans, M, K,
                                  ctypes.c_void_p(x), xdt, x_layout, N, nb, ctypes.c_void_p(bias), ctypes.c_void_p(y),
                                  ydt, ctypes.c_void_p(ws), ws_bytes, None)


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
    (dict(trans=2), ERR_ARG, b"trans_w"),
    (dict(x_layout=1, nb=2), ERR_ARG, b"nb = 1"),
    (dict(x_layout=2), ERR_ARG, b"x_layout"),
    (dict(xdt=DT_F32), ERR_ARG, b"x_dtype"),
    (dict(xdt=3), ERR_ARG, b"x_dtype"),
    (dict(xdt=DT_F16, ydt=DT_BF16), ERR_ARG, b"y_dtype"),
    (dict(ydt=7), ERR_ARG, b"y_dtype"),
    (dict(meta=(AFFINE, 8, 0, 200)), ERR_ARG, b"zero_point"),              # -128 - 200 is past bf16's 256
    (dict(meta=(AFFINE, 8, 0, -3000), xdt=DT_F16, ydt=DT_F16), ERR_ARG, b"zero_point"),
    (dict(codes=0x1004), ERR_ARG, b"16-byte"),
    (dict(x=0x10001), ERR_ARG, b"x must be aligned"),
    (dict(y=0x20001), ERR_ARG, b"y must be aligned"),
    (dict(y=0x20002, ydt=DT_F32), ERR_ARG, b"y must be aligned"),
    (dict(bias=0x30002), ERR_ARG, b"bias"),
    (dict(M=1 << 30), ERR_ARG, b"range"),
    (dict(K=(1 << 24) + 1), ERR_ARG, b"range"),
    (dict(M=512, K=1141, N=4, ws_bytes=16), ERR_WORKSPACE, b"workspace"),
    (dict(M=512, K=1141, N=4, ws=0, ws_bytes=1 << 30), ERR_WORKSPACE, b"workspace"),
    # tensor_minmax needs the partial column sums behind the images: the float size is short by them
    (dict(meta=(MINMAX, 4), M=512, K=1141, N=4, ws_bytes=18 * 512 * 4 * 4), ERR_WORKSPACE, b"workspace"),
])
def test_packed_hgemm_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    assert _call(lib, **kw) == status
    err = lib.admmq_last_error()
    assert word in err
    if status == ERR_ARG:
        assert b"packed_hgemm" in err


def _ws_formula(scheme, M, K, N, nb):
    """The header's formula: admmq_packed_gemm's plan (K pieces of kp = max(64, 32 ceil(K / 1024)); parallel, one
    float32 partial image of C M elements per piece, with more than one piece and fewer than 256 tiles), and for
    tensor_minmax in that regime 4 np C bytes more; 0 out of range."""
    if min(M, K, N, nb) <= 0 or M > 1 << 22 or N > 1 << 30 or nb > 1 << 30 or nb * N > 1 << 30:
        return 0
    if K > 1 << 24 or M * K >= 1 << 40:
        return 0
    kp = max(64, 32 * -(-K // 1024))
    pieces = -(-K // kp)
    tiles = -(-M // 64) * -(-(nb * N) // 64)
    if pieces > 1 and tiles < 256:
        return pieces * (nb * N * M) * 4 + (pieces * nb * N * 4 if scheme == MINMAX else 0)
    return 0


def test_workspace_sizes_match_the_closed_formula(lib):
    f = lib.admmq_packed_hgemm_workspace_size
    ks = [1, 63, 64, 65, 2048, 2049, 65536, 65537]
    mnb = [(8, 4, 1), (65, 129, 1), (64 * 255, 64, 1), (64 * 255 + 1, 64, 1), (64, 64 * 255, 1), (64, 64 * 255 + 1, 1),
           (960, 1088, 1), (960, 1089, 1), (1024, 1024, 1), (320, 3264, 1), (134, 65, 3), (512, 7, 2)]
    grid = [(M, K, N, nb) for K in ks for (M, N, nb) in mnb]
    grid += [(1 << 22, 65, 1, 1), ((1 << 22) + 1, 65, 1, 1), (8, 1 << 24, 4, 1), (8, (1 << 24) + 1, 4, 1),
             (8, 128, 1 << 30, 1), (8, 128, (1 << 30) + 1, 1), (8, 128, 1, 1 << 30), (8, 128, 1, (1 << 30) + 1),
             (8, 128, 1 << 20, 1 << 10), (8, 128, 1 << 20, (1 << 10) + 1), (1 << 22, (1 << 18) - 1, 1, 1),
             (1 << 22, 1 << 18, 1, 1), (0, 8, 8, 1), (8, 0, 8, 1), (8, 8, 0, 1), (8, 8, 8, 0), (8, 8, -1, 1)]
    for scheme, bits in ((MSE, 4), (MINMAX, 8), (SYMMETRIC, 3), (AFFINE, 5)):
        m = _meta(scheme, bits)
        for M, K, N, nb in grid:
            got = f(ctypes.byref(m), M, K, N, nb)
            assert got == _ws_formula(scheme, M, K, N, nb), (scheme, M, K, N, nb)
            assert got == f(ctypes.byref(m), M, K, N, nb)
            if scheme != MINMAX:
                assert got == lib.admmq_packed_gemm_workspace_size(M, K, N, nb)
    assert f(None, 8, 65, 4, 1) == 0
    m = _meta(MINMAX, 4)
    assert f(ctypes.byref(m), 8, 65, 4, 1) == 2 * 4 * 8 * 4 + 2 * 4 * 4


def test_header_declares_what_the_library_exports(lib):
    text = open(os.path.join(ROOT, "include", "admmq.h")).read()
    names = set(re.findall(r"\b(admmq_[a-z0-9_]+)\s*\(", text))
    for n in ("admmq_packed_hgemm", "admmq_packed_hgemm_workspace_size"):
        assert n in names and hasattr(lib, n)
    for name, val in (("ADMMQ_DT_F32", 0), ("ADMMQ_DT_F16", 1), ("ADMMQ_DT_BF16", 2)):
        assert re.search(rf"#define {name} {val}\b", text)
    proto = re.search(r"int32_t admmq_packed_hgemm\(([^;]*)\);", text).group(1)
    args = [a.strip() for a in " ".join(proto.split()).split(",")]
    assert len(args) == 16 == len(lib.admmq_packed_hgemm.argtypes)
    assert [a.split()[-1].lstrip("*") for a in args] == ["codes", "meta", "trans_w", "M", "K", "x", "x_dtype", "x_layout",
                                                         "N", "nb", "bias", "y", "y_dtype", "workspace",
                                                         "workspace_bytes", "stream"]
    proto = re.search(r"size_t\s+admmq_packed_hgemm_workspace_size\(([^;]*)\);", text).group(1)
    assert len(proto.split(",")) == 5 == len(lib.admmq_packed_hgemm_workspace_size.argtypes)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_meta_kernel_gives_shapes_and_dtypes(dtype):
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=m)
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)
    for out_f32 in (False, True):
        want = torch.float32 if out_f32 else dtype
        y = ops.packed_hgemm(codes, words, False, 64, 134, torch.empty(3, 134, 7, 5, device=m, dtype=dtype), 0, None, out_f32)
        assert tuple(y.shape) == (3, 64, 7, 5) and y.dtype == want
        y = ops.packed_hgemm(codes, words, True, 134, 64, torch.empty(3, 64, 7, 5, device=m, dtype=dtype), 0, None, out_f32)
        assert tuple(y.shape) == (3, 134, 7, 5) and y.dtype == want
        y = ops.packed_hgemm(codes, words, False, 64, 134, torch.empty(2, 5, 134, device=m, dtype=dtype), 1, None, out_f32)
        assert tuple(y.shape) == (2, 5, 64) and y.dtype == want
        y = ops.packed_hgemm(codes, words, True, 134, 64, torch.empty(64, device=m, dtype=dtype), 1,
                             torch.empty(134, device=m), out_f32)
        assert tuple(y.shape) == (134,) and y.dtype == want
    with pytest.raises(RuntimeError, match="x must be"):
        ops.packed_hgemm(codes, words, False, 64, 134, torch.empty(3, 64, 7, 5, device=m, dtype=dtype), 0, None, False)
    with pytest.raises(RuntimeError, match="float16 or bfloat16"):
        ops.packed_hgemm(codes, words, False, 64, 134, torch.empty(2, 134, device=m), 1, None, False)


def _host_packed(shape, bits=4):
    from admmq import PackedTensor
    from admmq.packed import packed_bytes
    n = shape[0] * shape[1]
    return PackedTensor(codes=torch.zeros(packed_bytes(n, bits), dtype=torch.uint8), shape=tuple(shape), bits=bits,
                        qscheme="tensor_symmetric", scale=0.25, zero_point=0, mn=0.0, rng=0.0, index=-1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_cpu_tensors_raise(dtype):
    import admmq
    from admmq import export
    p = _host_packed((6, 10))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_linear(torch.zeros(3, 10, dtype=dtype), p)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_conv1x1(torch.zeros(2, 10, 4, 4, dtype=dtype), p, stride=2, out_dtype=torch.float32)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        export.PackedLinear(p).half()(torch.zeros(3, 10, dtype=dtype))
    from admmq import PackedLowRank
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_lowrank_linear(torch.zeros(3, 10, dtype=dtype), PackedLowRank(p, torch.zeros(6, 2), torch.zeros(2, 10)))


class _FakeGpuTensor(torch.Tensor):
    """A host tensor that reports device 'cuda': the dtype and argument refusals of the Python layer come
    before any device call, and are reached without a GPU."""
    @property
    def device(self):
        return torch.device("cuda:0")


def _fake(t):
    return t.as_subclass(_FakeGpuTensor)


def test_act_with_a_half_x_and_other_dtypes_are_refused():
    from admmq.packed import _meta_words, packed_gemm
    p = _host_packed((6, 10))
    codes, words = _fake(p.codes), _meta_words(p)
    for dtype in (torch.bfloat16, torch.float16):
        x = _fake(torch.zeros(3, 10, dtype=dtype))
        with pytest.raises(ValueError, match="act="):
            packed_gemm(codes, words, False, 6, 10, x, 1, None, (4, -1.0, 1.0))
        with pytest.raises(ValueError, match="out_dtype"):
            packed_gemm(codes, words, False, 6, 10, x, 1, None, None, torch.float64)
        other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
        with pytest.raises(ValueError, match="out_dtype"):
            packed_gemm(codes, words, False, 6, 10, x, 1, None, None, other)
        with pytest.raises(TypeError, match="bias must be float32 or x's dtype"):
            packed_gemm(codes, words, False, 6, 10, x, 1, _fake(torch.zeros(6, dtype=other)))
    # every other dtype keeps the float path's TypeError
    for dtype in (torch.float64, torch.int8):
        with pytest.raises(TypeError, match=f"float32 tensors required, got {dtype}"):
            packed_gemm(codes, words, False, 6, 10, _fake(torch.zeros(3, 10, dtype=dtype)), 1)
    with pytest.raises(ValueError, match="float32 result"):
        packed_gemm(codes, words, False, 6, 10, _fake(torch.zeros(3, 10)), 1, None, None, torch.bfloat16)


def test_modules_keep_codes_and_record_through_half(tmp_path):
    from admmq import PackedLowRank, export
    p = _host_packed((6, 10), bits=3)
    p.codes.copy_(torch.arange(p.codes.numel(), dtype=torch.uint8))
    lin = export.PackedLinear(p, bias=torch.arange(6, dtype=torch.float32))
    state = lin.get_extra_state()
    words = lin._meta.clone()
    lin.half()
    assert lin.codes.dtype == torch.uint8 and torch.equal(lin.codes, p.codes)
    assert lin.bias.dtype == torch.float16 and not lin.bias.requires_grad
    assert lin.get_extra_state() == state and torch.equal(lin._meta, words)
    sd = lin.state_dict()
    assert set(sd) == {"codes", "bias", "_extra_state"} and sd["bias"].dtype == torch.float16
    path = str(tmp_path / "half.pt")
    torch.save(sd, path)
    fresh = export.PackedLinear(_host_packed((6, 10), bits=3), bias=torch.zeros(6)).bfloat16()
    fresh.load_state_dict(torch.load(path, weights_only=True))
    assert torch.equal(fresh.codes, p.codes) and fresh.bias.dtype == torch.bfloat16
    assert torch.equal(fresh.bias.float(), torch.arange(6, dtype=torch.float32))
    assert fresh.get_extra_state() == state
    conv = export.PackedConv1x1(p, transpose=True, stride=2).bfloat16()
    assert conv.codes.dtype == torch.uint8 and conv.bias is None and conv.get_extra_state()["bits"] == 3
    qlr = export.PackedLowRankLinear(PackedLowRank(p, torch.ones(6, 2), torch.ones(2, 10)), bias=torch.ones(6)).half()
    assert qlr.codes.dtype == torch.uint8 and qlr.L.dtype == torch.float16 and qlr.Rt.dtype == torch.float16
    assert qlr.get_extra_state()["rank"] == 2
    seq = export.build_cp2conv_layer(5, [_host_packed((12, 5)), _host_packed((8, 5))], torch.zeros(12), 8, 12, 0, 1).half()
    assert seq.conv1.codes.dtype == torch.uint8 and seq.conv2.bias.dtype == torch.float16
