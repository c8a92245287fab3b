"""Half-precision fused depthwise + 1x1 stage, host side (no GPU): every refusal of
admmq_packed_hdwgemm comes back with its status and its own text before any device call (made-up device
addresses), the workspace query equals the half GEMM's, the header declares what the library exports, the
Meta kernel propagates shape and dtype, and the wrappers refuse CPU tensors and other dtypes as documented."""
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


def _call(lib, meta="ok", codes=0x1000, t=0x10000, taps=0x30000, y=0x20000, M=8, K=8, nb=1, H=6, W=6, k=(3, 3), s=(1, 1),
          p=(1, 1), bias=0, ws=0x100000, ws_bytes=1 << 20, tdt=DT_BF16, ydt=DT_BF16):
    m = _meta() if meta == "ok" else meta
    return lib.admmq_packed_hdwgemm(ctypes.c_void_p(codes), ctypes.byref(m) if m is not None else None, M, K,
                                    ctypes.c_void_p(t), tdt, nb, H, W, ctypes.c_void_p(taps), k[0], k[1], s[0], s[1], p[0],
                                    p[1], ctypes.c_void_p(bias), ctypes.c_void_p(y), ydt, ctypes.c_void_p(ws), ws_bytes, None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(codes=0), ERR_ARG, b"NULL"),
    (dict(t=0), ERR_ARG, b"NULL"),
    (dict(taps=0), ERR_ARG, b"NULL"),
    (dict(y=0), ERR_ARG, b"NULL"),
    (dict(meta=None), ERR_ARG, b"NULL"),
    (dict(M=0), ERR_ARG, b"positive"),
    (dict(K=-3), ERR_ARG, b"positive"),
    (dict(H=0), ERR_ARG, b"positive"),
    (dict(nb=0), ERR_ARG, b"positive"),
    (dict(meta=(SYMMETRIC, 9)), ERR_ARG, b"bits"),
    (dict(meta=(4, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(MINMAX, 1)), ERR_ARG, b"1 bit"),
    (dict(meta=(AFFINE, 4, 2)), ERR_ARG, b"bad"),
    (dict(k=(8, 3)), ERR_ARG, b"kernel size"),
    (dict(s=(0, 1)), ERR_ARG, b"stride"),
    (dict(p=(3, 1)), ERR_ARG, b"padding"),
    (dict(H=1, W=1, k=(3, 3), p=(0, 0)), ERR_ARG, b"does not fit"),
    (dict(tdt=DT_F32, ydt=DT_F32), ERR_ARG, b"t_dtype must be"),
    (dict(tdt=3), ERR_ARG, b"t_dtype must be"),
    (dict(tdt=DT_F16, ydt=DT_BF16), ERR_ARG, b"y_dtype"),
    (dict(meta=(AFFINE, 8, 0, 200)), ERR_ARG, b"zero_point"),              # -128 - 200 is past bf16's 256
    (dict(meta=(AFFINE, 8, 0, -3000), tdt=DT_F16, ydt=DT_F16), ERR_ARG, b"zero_point"),
    (dict(codes=0x1004), ERR_ARG, b"16-byte"),
    (dict(t=0x10001), ERR_ARG, b"t must be aligned"),
    (dict(y=0x20001), ERR_ARG, b"y must be aligned"),
    (dict(y=0x20002, ydt=DT_F32), ERR_ARG, b"y must be aligned"),
    (dict(bias=0x30002), ERR_ARG, b"bias"),
    (dict(taps=0x30002), ERR_ARG, b"taps must be float aligned"),
    (dict(M=1 << 30), ERR_ARG, b"range"),
    (dict(K=1 << 22, H=1 << 10, W=1 << 10, nb=4), ERR_ARG, b"2^40"),
    (dict(M=512, K=1141, ws_bytes=16), ERR_WORKSPACE, b"workspace"),
    (dict(M=512, K=1141, ws=0, ws_bytes=1 << 30), ERR_WORKSPACE, b"workspace"),
    (dict(meta=(MINMAX, 4), M=512, K=1141, ws_bytes=18 * 512 * 36 * 4), ERR_WORKSPACE, b"workspace"),
])
def test_packed_hdwgemm_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    assert _call(lib, **kw) == status
    err = lib.admmq_last_error()
    assert word in err
    if status == ERR_ARG:
        assert b"packed_hdwgemm" in err


def test_workspace_size_is_the_half_gemms(lib):
    f, h = lib.admmq_packed_hdwgemm_workspace_size, lib.admmq_packed_hgemm_workspace_size
    seen = set()
    for scheme, bits in ((MSE, 4), (MINMAX, 8), (SYMMETRIC, 3), (AFFINE, 5)):
        m = ctypes.byref(_meta(scheme, bits))
        for M in (8, 65, 512, 64 * 255 + 1):
            for K in (1, 64, 65, 1141, 2049):
                for Ho, Wo, nb in ((1, 1, 1), (4, 4, 1), (7, 7, 3), (31, 31, 6), (56, 56, 64)):
                    got = f(m, M, K, Ho, Wo, nb)
                    assert got == h(m, M, K, Ho * Wo, nb), (scheme, M, K, Ho, Wo, nb)
                    seen.add(got > 0)
        assert f(m, 8, 65, 0, 4, 1) == 0 and f(m, 8, 65, 4, (1 << 30) + 1, 1) == 0 and f(m, 0, 65, 4, 4, 1) == 0
    assert seen == {False, True} and f(None, 8, 65, 2, 2, 1) == 0


def test_header_declares_what_the_library_exports(lib):
    text = open(os.path.join(ROOT, "include", "admmq.h")).read()
    proto = re.search(r"int32_t admmq_packed_hdwgemm\(([^;]*)\);", text).group(1)
    args = [a.strip().split()[-1].lstrip("*") for a in " ".join(proto.split()).split(",")]
    assert args == ["codes", "meta", "M", "K", "t", "t_dtype", "nb", "H", "W", "taps", "kh", "kw", "sh", "sw", "ph", "pw",
                    "bias", "y", "y_dtype", "workspace", "workspace_bytes", "stream"]
    assert len(args) == len(lib.admmq_packed_hdwgemm.argtypes)
    proto = re.search(r"size_t\s+admmq_packed_hdwgemm_workspace_size\(([^;]*)\);", text).group(1)
    assert len(proto.split(",")) == 6 == len(lib.admmq_packed_hdwgemm_workspace_size.argtypes)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_meta_kernel_gives_shapes_and_dtypes(dtype):
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=m)
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)
    x, taps = torch.empty(3, 134, 7, 9, device=m, dtype=dtype), torch.empty(9, 134, device=m)
    for out_f32 in (False, True):
        y = ops.packed_hdwgemm(codes, words, 64, 134, x, taps, 3, 3, 2, 1, 1, 1, None, out_f32)
        assert tuple(y.shape) == (3, 64, 4, 9) and y.dtype == (torch.float32 if out_f32 else dtype)
    with pytest.raises(RuntimeError, match="float16 or bfloat16"):
        ops.packed_hdwgemm(codes, words, 64, 134, x.float(), taps, 3, 3, 1, 1, 1, 1, None, False)
    with pytest.raises(RuntimeError, match="taps must be"):
        ops.packed_hdwgemm(codes, words, 64, 134, x, taps[:8], 3, 3, 1, 1, 1, 1, None, False)
    with pytest.raises(RuntimeError, match="padding"):
        ops.packed_hdwgemm(codes, words, 64, 134, x, taps, 3, 3, 1, 1, 3, 1, None, False)


class _FakeGpuTensor(torch.Tensor):
    """A host tensor that reports device 'cuda': the refusals of the Python layer come before any device call."""
    @property
    def device(self):
        return torch.device("cuda:0")


def _fake(t):
    return t.as_subclass(_FakeGpuTensor)


def _host_packed(shape, bits=4):
    from admmq import PackedTensor
    from admmq.packed import packed_bytes
    return PackedTensor(codes=torch.zeros(packed_bytes(shape[0] * shape[1], bits), dtype=torch.uint8), shape=tuple(shape),
                        bits=bits, qscheme="tensor_symmetric", scale=0.25, zero_point=0, mn=0.0, rng=0.0, index=-1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_wrapper_refusals(dtype, monkeypatch):
    import admmq
    from admmq import _lib, export
    from admmq.packed import _meta_words, packed_dwgemm
    p = _host_packed((6, 10))
    x, taps = torch.zeros(2, 10, 4, 4, dtype=dtype), torch.zeros(9, 10)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_depthwise_conv1x1(x, taps, p, kernel_size=3, padding=1)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        export.PackedDepthwiseConv1x1(p, taps, kernel_size=3, padding=1).to(dtype)(x)
    codes, words, other = _fake(p.codes), _meta_words(p), torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    call = lambda xx, tt, **kw: packed_dwgemm(codes, words, 6, 10, _fake(xx), _fake(tt), 3, 1, 1, **kw)
    for kw in (dict(act=(4, -1.0, 1.0)), dict(mid_act=(4, -1.0, 1.0))):
        with pytest.raises(ValueError, match="act="):
            call(x, taps, **kw)
    for od in (torch.float64, other):
        with pytest.raises(ValueError, match="out_dtype"):
            call(x, taps, out_dtype=od)
    with pytest.raises(TypeError, match="taps must be float32 or x's dtype"):
        call(x, taps.to(other))
    with pytest.raises(TypeError, match="bias must be float32 or x's dtype"):
        call(x, taps, bias=_fake(torch.zeros(6, dtype=other)))
    # every other dtype keeps the float path's TypeError; a float32 x keeps its refusals and its entry point
    for bad in (torch.float64, torch.int8):
        with pytest.raises(TypeError, match=f"float32 tensors required, got {bad}"):
            call(x.to(bad), taps)
    with pytest.raises(TypeError, match=f"float32 tensors required, got {dtype}"):
        call(x.float(), taps.to(dtype))
    with pytest.raises(ValueError, match="float32 result"):
        call(x.float(), taps, out_dtype=dtype)
    seen = []
    monkeypatch.setattr(_lib, "use_ops", lambda: True)
    monkeypatch.setattr(_lib, "ops", lambda: type("Ops", (), {"packed_dwgemm": lambda *a: seen.append(a) or "f32"}))
    assert call(x.float(), taps) == "f32" and len(seen) == 1
