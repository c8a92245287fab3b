"""Skinny packed GEMV, host side (no GPU): every refusal of admmq_packed_gemv comes back with
its status and its own text before any device call (made-up device addresses), the workspace query is a pure
function that matches the written plan, the header declares what the library exports, the Meta kernel
propagates shape and dtype, CPU tensors raise, and skinny=True with act= is refused."""
import ctypes
import os
import re

import pytest
import torch

from test_packed_hgemm_host import (AFFINE, DT_BF16, DT_F16, DT_F32, ERR_ARG, ERR_WORKSPACE, MINMAX, MSE, ROOT, SYMMETRIC,
                                    _host_packed, _meta)


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    return _lib.load()


def _call(lib, meta="ok", codes=0x1000, x=0x10000, y=0x20000, M=8, K=8, N=4, bias=0, ws=0x100000, ws_bytes=1 << 20, trans=0,
          xdt=DT_BF16, ydt=DT_BF16):
    m = _meta() if meta == "ok" else meta
    return lib.admmq_packed_gemv(ctypes.c_void_p(codes), ctypes.byref(m) if m is not None else None, trans, M, K,
                                 ctypes.c_void_p(x), xdt, N, ctypes.c_void_p(bias), ctypes.c_void_p(y), ydt,
                                 ctypes.c_void_p(ws), ws_bytes, None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(codes=0), ERR_ARG, b"NULL"),
    (dict(meta=None), ERR_ARG, b"NULL"),
    (dict(M=0), ERR_ARG, b"positive"),
    (dict(N=0), ERR_ARG, b"N must be 1..8"),
    (dict(N=9), ERR_ARG, b"N must be 1..8"),
    (dict(meta=(MSE, 0)), ERR_ARG, b"bits"),
    (dict(meta=(4, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(MINMAX, 1)), ERR_ARG, b"1 bit"),
    (dict(meta=(AFFINE, 4, 2)), ERR_ARG, b"bad"),
    (dict(trans=2), ERR_ARG, b"trans_w"),
    (dict(xdt=3), ERR_ARG, b"x_dtype"),
    (dict(xdt=DT_F16, ydt=DT_BF16), ERR_ARG, b"y_dtype"),
    (dict(xdt=DT_F32, ydt=DT_F16), ERR_ARG, b"y_dtype"),
    (dict(meta=(AFFINE, 8, 0, 200)), ERR_ARG, b"zero_point"),              # -128 - 200 is past bf16's 256
    (dict(meta=(AFFINE, 8, 0, -3000), xdt=DT_F16, ydt=DT_F16), ERR_ARG, b"zero_point"),
    (dict(codes=0x1004), ERR_ARG, b"16-byte"),
    (dict(x=0x10001), ERR_ARG, b"x must be aligned"),
    (dict(x=0x10002, xdt=DT_F32, ydt=DT_F32), ERR_ARG, b"x must be aligned"),
    (dict(y=0x20002, ydt=DT_F32), ERR_ARG, b"y must be aligned"),
    (dict(bias=0x30002), ERR_ARG, b"bias"),
    (dict(M=1 << 30), ERR_ARG, b"range"),
    (dict(K=(1 << 24) + 1), ERR_ARG, b"range"),
    (dict(M=8, K=2048, N=4, ws_bytes=16), ERR_WORKSPACE, b"workspace"),
    (dict(M=8, K=2048, N=4, ws=0, ws_bytes=1 << 30), ERR_WORKSPACE, b"workspace"),
    (dict(M=8, K=2048, N=4, ws=0x100002), ERR_ARG, b"workspace must be float aligned"),
    # tensor_minmax needs the ranges' sums of x behind the partial sums: the scale schemes' size is short by them
    (dict(meta=(MINMAX, 4), M=8, K=2048, N=4, ws_bytes=2 * 4 * 8 * 4), ERR_WORKSPACE, b"workspace"),
])
def test_packed_gemv_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    assert _call(lib, **kw) == status
    err = lib.admmq_last_error()
    assert word in err
    if status == ERR_ARG:
        assert b"packed_gemv" in err


def test_workspace_query_is_pure_and_follows_the_plan(lib):
    """Named shapes of the plan: ns ranges give 4 ns N M bytes (+ 4 ns N for tensor_minmax), one
    launch gives 0; N only scales the size; out of range gives 0."""
    f = lib.admmq_packed_gemv_workspace_size
    m, mx = _meta(MSE, 4), _meta(MINMAX, 8)
    # (trans, M, K) -> ns: one launch from 256 tiles or within one range's minimum; else up to 16 ranges
    plan = {(0, 11008, 4096): 1, (0, 8161, 4096): 1, (0, 8160, 4096): 2, (0, 4096, 4096): 4, (0, 4096, 11008): 4,
            (0, 4096, 1024): 1, (0, 3, 1025): 2, (0, 3, 16500): 9, (1, 4096, 4096): 16, (1, 5, 129): 2, (1, 5, 128): 1,
            (1, 5, 8300): 13, (1, 65281, 4096): 1}
    for (trans, M, K), ns in plan.items():
        for N in (1, 3, 8):
            want = 4 * ns * N * M if ns > 1 else 0
            assert f(ctypes.byref(m), trans, M, K, N) == want == f(ctypes.byref(m), trans, M, K, N), (trans, M, K, N)
            assert f(ctypes.byref(mx), trans, M, K, N) == (want + 4 * ns * N if ns > 1 else 0)
    for args in [(2, 8, 2048, 4), (0, 0, 2048, 4), (0, 8, 0, 4), (0, 8, 2048, 0), (0, 8, 2048, 9), (0, (1 << 22) + 1, 65, 1),
                 (0, 8, (1 << 24) + 1, 4), (0, 1 << 22, 1 << 18, 1)]:
        assert f(ctypes.byref(m), *args) == 0, args
    assert f(None, 0, 8, 2048, 4) == 0


def test_header_declares_what_the_library_exports(lib):
    text = open(os.path.join(ROOT, "include", "admmq.h")).read()
    names = set(re.findall(r"\b(admmq_[a-z0-9_]+)\s*\(", text))
    for n in ("admmq_packed_gemv", "admmq_packed_gemv_workspace_size"):
        assert n in names and hasattr(lib, n)
    assert re.search(r"#define ADMMQ_GEMV_N_MAX 8\b", text)
    proto = re.search(r"int32_t admmq_packed_gemv\(([^;]*)\);", text).group(1)
    args = [a.strip() for a in " ".join(proto.split()).split(",")]
    assert len(args) == 14 == len(lib.admmq_packed_gemv.argtypes)
    proto = re.search(r"size_t\s+admmq_packed_gemv_workspace_size\(([^;]*)\);", text).group(1)
    assert len(proto.split(",")) == 5 == len(lib.admmq_packed_gemv_workspace_size.argtypes)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_meta_kernel_gives_shapes_and_dtypes(dtype):
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=m)
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)
    for out_f32 in (False, True):
        want = torch.float32 if out_f32 else dtype
        y = ops.packed_gemv(codes, words, False, 64, 134, torch.empty(2, 4, 134, device=m, dtype=dtype), None, out_f32)
        assert tuple(y.shape) == (2, 4, 64) and y.dtype == want
        y = ops.packed_gemv(codes, words, True, 134, 64, torch.empty(64, device=m, dtype=dtype), torch.empty(134, device=m), out_f32)
        assert tuple(y.shape) == (134,) and y.dtype == want
    with pytest.raises(RuntimeError, match="1..8 rows"):
        ops.packed_gemv(codes, words, False, 64, 134, torch.empty(9, 134, device=m, dtype=dtype), None, False)
    with pytest.raises(RuntimeError, match="float32, float16 or bfloat16"):
        ops.packed_gemv(codes, words, False, 64, 134, torch.empty(3, 134, device=m, dtype=torch.float64), None, False)


def test_cpu_tensors_raise_and_skinny_with_act_is_refused():
    import admmq
    from admmq import export
    from admmq.packed import _meta_words
    p = _host_packed((6, 10))
    assert "packed_gemv" in admmq.packed.__all__
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        x = torch.zeros(3, 10, dtype=dtype)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            admmq.packed_gemv(p.codes, _meta_words(p), False, 6, 10, x)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            admmq.packed_linear(x, p, skinny=True)
        lin = export.PackedLinear(p)
        lin.skinny = True
        assert "skinny" not in lin.state_dict() and "skinny" not in lin.get_extra_state() and "skinny=True" in repr(lin)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            lin(x)
        with pytest.raises(ValueError, match="skinny=True cannot be combined with act="):
            admmq.packed_linear(x, p, act=(4, -1.0, 1.0), skinny=True)
