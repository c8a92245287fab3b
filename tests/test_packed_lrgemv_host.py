"""Skinny quant + low-rank GEMV, host side (no GPU): every refusal of admmq_packed_lrgemv comes back
with its status and its own text before any device call (made-up device addresses), the workspace and plan
queries are pure functions that match the written plan, the header declares what the library exports, the Meta
kernel propagates shape and dtype, CPU tensors raise, and skinny=False leaves today's call path untouched."""
import ctypes
import os
import re

import pytest
import torch

from test_packed_hgemm_host import (AFFINE, DT_BF16, DT_F16, DT_F32, ERR_ARG, ERR_WORKSPACE, MINMAX, MSE, ROOT, _host_packed,
                                    _meta)


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    return _lib.load()


def _call(lib, meta="ok", codes=0x1000, L=0x40000, Rt=0x50000, fdt=DT_F32, r=8, x=0x10000, y=0x20000, M=8, K=8, N=4, bias=0,
          ws=0x100000, ws_bytes=1 << 20, xdt=DT_BF16, ydt=DT_BF16):
    m = _meta() if meta == "ok" else meta
    return lib.admmq_packed_lrgemv(ctypes.c_void_p(codes), ctypes.byref(m) if m is not None else None, M, K, ctypes.c_void_p(L),
                                   ctypes.c_void_p(Rt), fdt, r, ctypes.c_void_p(x), xdt, N, ctypes.c_void_p(bias),
                                   ctypes.c_void_p(y), ydt, ctypes.c_void_p(ws), ws_bytes, None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(codes=0), ERR_ARG, b"NULL"),
    (dict(meta=None), ERR_ARG, b"NULL"),
    (dict(L=0), ERR_ARG, b"NULL"),
    (dict(Rt=0), ERR_ARG, b"NULL"),
    (dict(x=0), ERR_ARG, b"NULL"),
    (dict(y=0), ERR_ARG, b"NULL"),
    (dict(K=0), ERR_ARG, b"positive"),
    (dict(N=0), ERR_ARG, b"N must be 1..8"),
    (dict(N=9), ERR_ARG, b"N must be 1..8"),
    (dict(r=0), ERR_ARG, b"rank r must be 1..256"),
    (dict(r=257), ERR_ARG, b"rank r must be 1..256"),
    (dict(meta=(MSE, 0)), ERR_ARG, b"bits"),
    (dict(meta=(4, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(MINMAX, 1)), ERR_ARG, b"1 bit"),
    (dict(meta=(AFFINE, 4, 2)), ERR_ARG, b"bad"),
    (dict(xdt=3), ERR_ARG, b"x_dtype"),
    (dict(xdt=DT_F16, ydt=DT_BF16), ERR_ARG, b"y_dtype"),
    (dict(fdt=3), ERR_ARG, b"f_dtype"),
    (dict(fdt=DT_F16), ERR_ARG, b"f_dtype"),                               # x is bfloat16
    (dict(fdt=DT_BF16, xdt=DT_F32, ydt=DT_F32), ERR_ARG, b"f_dtype"),
    (dict(meta=(AFFINE, 8, 0, 200)), ERR_ARG, b"zero_point"),
    (dict(codes=0x1004), ERR_ARG, b"16-byte"),
    (dict(x=0x10001), ERR_ARG, b"x must be aligned"),
    (dict(y=0x20002, ydt=DT_F32), ERR_ARG, b"y must be aligned"),
    (dict(L=0x40002), ERR_ARG, b"L and Rt must be aligned"),
    (dict(Rt=0x50001, fdt=DT_BF16), ERR_ARG, b"L and Rt must be aligned"),
    (dict(bias=0x30002), ERR_ARG, b"bias"),
    (dict(M=1 << 30), ERR_ARG, b"range"),
    (dict(K=(1 << 24) + 1), ERR_ARG, b"range"),
    (dict(ws_bytes=4 * 4 * 8 - 1), ERR_WORKSPACE, b"workspace"),           # t alone: one launch needs 4 nsd N r bytes
    (dict(ws=0), ERR_WORKSPACE, b"workspace"),
    (dict(ws=0x100002), ERR_ARG, b"workspace must be float aligned"),
    # the K-split plan: t, ns + 1 images of [N, M], and tensor_minmax's sums of x behind them
    (dict(meta=(MINMAX, 4), M=8, K=2048, N=4, ws_bytes=4 * (8 * 4 * 8 + 3 * 4 * 8 + 2 * 4) - 1), ERR_WORKSPACE, b"workspace"),
])
def test_packed_lrgemv_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    assert _call(lib, **kw) == status
    err = lib.admmq_last_error()
    assert word in err
    if status == ERR_ARG:
        assert b"packed_lrgemv" in err


def test_plan_and_workspace_queries_are_pure_and_follow_the_plan(lib):
    """Named shapes: ns is admmq_packed_gemv's; nsd = ranges of 256 ceil(ceil(K / want) / 256) k,
    want = min(ceil(256 / ceil(r / 4)), 16, ceil(K / 256)); bytes = 4 nsd N r (+ 4 (ns + 1) N M (+ 4 ns N))."""
    size, plan = lib.admmq_packed_lrgemv_workspace_size, lib.admmq_packed_lrgemv_plan
    m, mx = _meta(MSE, 4), _meta(MINMAX, 8)
    named = {(4096, 4096, 8): (4, 16), (4096, 4096, 64): (4, 16), (11008, 4096, 64): (1, 16), (4096, 11008, 8): (4, 15),
             (4096, 11008, 256): (4, 4), (64, 134, 33): (1, 1), (3, 1025, 9): (2, 5), (5, 257, 1): (1, 2), (5, 256, 1): (1, 1)}
    for (M, K, r), (ns, nsd) in named.items():
        out = (ctypes.c_int32 * 3)()
        assert plan(ctypes.byref(m), M, K, r, out) == 0 and tuple(out) == (ns, nsd, 3 if ns > 1 else 2), (M, K, r, tuple(out))
        assert (ns > 1) == (lib.admmq_packed_gemv_workspace_size(ctypes.byref(m), 0, M, K, 1) > 0)
        for N in (1, 3, 8):
            want = 4 * nsd * N * r + (4 * (ns + 1) * N * M if ns > 1 else 0)
            assert size(ctypes.byref(m), M, K, N, r) == want == size(ctypes.byref(m), M, K, N, r), (M, K, N, r)
            assert size(ctypes.byref(mx), M, K, N, r) == want + (4 * ns * N if ns > 1 else 0)
    out = (ctypes.c_int32 * 3)(7, 7, 7)
    for args in [(0, 2048, 4, 8), (8, 0, 4, 8), (8, 2048, 0, 8), (8, 2048, 9, 8), (8, 2048, 4, 0), (8, 2048, 4, 257),
                 ((1 << 22) + 1, 65, 1, 8), (8, (1 << 24) + 1, 4, 8)]:
        assert size(ctypes.byref(m), *args) == 0, args
        if args[2] == 4:
            assert plan(ctypes.byref(m), args[0], args[1], args[3], out) == ERR_ARG and tuple(out) == (7, 7, 7)
    assert size(None, 8, 2048, 4, 8) == 0 and plan(None, 8, 2048, 8, out) == ERR_ARG
    assert plan(ctypes.byref(m), 8, 2048, 8, None) == ERR_ARG


def test_header_declares_what_the_library_exports(lib):
    text = open(os.path.join(ROOT, "include", "admmq.h")).read()
    names = set(re.findall(r"\b(admmq_[a-z0-9_]+)\s*\(", text))
    for n, nargs in (("admmq_packed_lrgemv", 17), ("admmq_packed_lrgemv_workspace_size", 5), ("admmq_packed_lrgemv_plan", 5)):
        assert n in names and hasattr(lib, n)
        proto = re.search(r"\b%s\(([^;]*)\);" % n, text).group(1)
        assert len(proto.split(",")) == nargs == len(getattr(lib, n).argtypes)
    assert "c = 29" in text   # the bound's constant is stated next to the contract


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_meta_kernel_gives_shapes_and_dtypes(dtype):
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=m)
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)
    L, Rt = torch.empty(64, 5, device=m), torch.empty(5, 134, device=m)
    for out_f32 in (False, True):
        want = torch.float32 if out_f32 else dtype
        y = ops.packed_lrgemv(codes, words, 64, 134, L, Rt, torch.empty(2, 4, 134, device=m, dtype=dtype), None, out_f32)
        assert tuple(y.shape) == (2, 4, 64) and y.dtype == want
        y = ops.packed_lrgemv(codes, words, 64, 134, L.to(dtype), Rt.to(dtype), torch.empty(134, device=m, dtype=dtype),
                              torch.empty(64, device=m), out_f32)
        assert tuple(y.shape) == (64,) and y.dtype == want
    x3 = torch.empty(3, 134, device=m, dtype=dtype)
    with pytest.raises(RuntimeError, match="1..8 rows"):
        ops.packed_lrgemv(codes, words, 64, 134, L, Rt, torch.empty(9, 134, device=m, dtype=dtype), None, False)
    with pytest.raises(RuntimeError, match="rank r must be 1..256"):
        ops.packed_lrgemv(codes, words, 64, 134, torch.empty(64, 257, device=m), torch.empty(257, 134, device=m), x3, None, False)
    with pytest.raises(RuntimeError, match="both be float32 or both of x's dtype"):
        ops.packed_lrgemv(codes, words, 64, 134, L.double(), Rt.double(), x3, None, False)
    with pytest.raises(RuntimeError, match="float32, float16 or bfloat16"):
        ops.packed_lrgemv(codes, words, 64, 134, L, Rt, x3.double(), None, False)


def test_cpu_tensors_raise_and_skinny_false_is_todays_call(monkeypatch):
    import admmq
    from admmq import export, packed
    from admmq.packed import _meta_words
    p = admmq.PackedLowRank(q=_host_packed((6, 10)), L=torch.zeros(6, 2), Rt=torch.zeros(2, 10))
    assert "packed_lrgemv" in packed.__all__ and admmq.packed_lrgemv is packed.packed_lrgemv
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        x = torch.zeros(3, 10, dtype=dtype)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            admmq.packed_lrgemv(p.q.codes, _meta_words(p.q), 6, 10, p.L, p.Rt, x)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            admmq.packed_lowrank_linear(x, p, skinny=True)
        lin = export.PackedLowRankLinear(p)
        lin.skinny = True
        assert "skinny" not in lin.state_dict() and "skinny" not in lin.get_extra_state() and "skinny=True" in repr(lin)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            lin(x)
    # without the flag (and with it, past 8 rows) the call is packed_lrgemm's, arguments unchanged; 8 rows with it: packed_lrgemv's
    calls = []
    monkeypatch.setattr(packed, "packed_lrgemm", lambda *a: calls.append(("lrgemm", a)))
    monkeypatch.setattr(packed, "packed_lrgemv", lambda *a: calls.append(("lrgemv", a)))
    x8, x9, bias = torch.zeros(2, 4, 10), torch.zeros(9, 10), torch.zeros(6)
    packed.packed_lowrank_linear(x8, p, bias, torch.float32)
    packed.packed_lowrank_linear(x9, p, bias, None, skinny=True)
    packed.packed_lowrank_linear(x8, p, bias, None, skinny=True)
    assert [c[0] for c in calls] == ["lrgemm", "lrgemm", "lrgemv"]
    for (_, a), x, od in zip(calls, (x8, x9, x8), (torch.float32, None, None)):
        assert a[0] is p.q.codes and a[2:4] == (6, 10) and a[4] is p.L and a[5] is p.Rt and a[6] is x and a[7] is bias and a[8] is od
