"""Half-precision fused quant + low-rank GEMM, host side (no GPU): every refusal of
admmq_packed_hlrgemm comes back with its status and its own text before any device call (made-up device addresses),
the workspace and plan queries are pure and match the written plan, the header declares what the library exports,
the Meta kernel propagates shape and dtype, CPU tensors raise, and without fused=True (or with it on a float32 x)
packed_lowrank_linear makes today's packed_lrgemm call."""
import ctypes
import os
import re

import pytest
import torch

from test_packed_hgemm_host import (AFFINE, DT_BF16, DT_F16, DT_F32, ERR_ARG, ERR_WORKSPACE, MINMAX, MSE, ROOT, _host_packed,
                                    _meta)

# (M, K, N, r) -> (np, parallel, nsd): the shapes of tests/test_gpu_packed_hlrgemm.py, and the timing tool's
NAMED = {(64, 134, 37, 1): (3, 1, 3), (64, 134, 37, 256): (3, 1, 3), (134, 134, 70, 24): (3, 1, 3), (33, 65, 9, 5): (2, 1, 2),
         (1, 7, 1, 3): (1, 0, 1), (1024, 65, 1024, 9): (2, 0, 2), (4096, 4096, 16, 8): (32, 1, 8), (4096, 4096, 512, 64): (32, 0, 8),
         (11008, 4096, 64, 64): (32, 1, 8), (4096, 11008, 512, 64): (32, 0, 8), (4096, 4096, 4096, 256): (32, 0, 1)}


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    return _lib.load()


def _call(lib, meta="ok", codes=0x1000, L=0x40000, Rt=0x50000, fdt=DT_F32, r=8, x=0x10000, y=0x20000, M=8, K=8, N=4, bias=0,
          ws=0x100000, ws_bytes=1 << 20, xdt=DT_BF16, ydt=DT_BF16):
    m = _meta() if meta == "ok" else meta
    return lib.admmq_packed_hlrgemm(ctypes.c_void_p(codes), ctypes.byref(m) if m is not None else None, M, K, ctypes.c_void_p(L),
                                    ctypes.c_void_p(Rt), fdt, r, ctypes.c_void_p(x), xdt, N, ctypes.c_void_p(bias),
                                    ctypes.c_void_p(y), ydt, ctypes.c_void_p(ws), ws_bytes, None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(codes=0), ERR_ARG, b"NULL"), (dict(meta=None), ERR_ARG, b"NULL"), (dict(L=0), ERR_ARG, b"NULL"),
    (dict(Rt=0), ERR_ARG, b"NULL"), (dict(x=0), ERR_ARG, b"NULL"), (dict(y=0), ERR_ARG, b"NULL"),
    (dict(M=0), ERR_ARG, b"positive"), (dict(K=0), ERR_ARG, b"positive"), (dict(N=0), ERR_ARG, b"positive"),
    (dict(r=0), ERR_ARG, b"rank r must be 1..256"), (dict(r=257), ERR_ARG, b"rank r must be 1..256"),
    (dict(meta=(MSE, 0)), ERR_ARG, b"bits"),
    (dict(meta=(4, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(MINMAX, 1)), ERR_ARG, b"1 bit"),
    (dict(meta=(AFFINE, 4, 2)), ERR_ARG, b"bad"),
    (dict(xdt=DT_F32, ydt=DT_F32), ERR_ARG, b"x_dtype must be ADMMQ_DT_F16 or ADMMQ_DT_BF16"),
    (dict(xdt=3), ERR_ARG, b"x_dtype"),
    (dict(xdt=DT_F16, ydt=DT_BF16), ERR_ARG, b"y_dtype"),
    (dict(meta=(AFFINE, 8, 0, 200)), ERR_ARG, b"zero_point"),
    (dict(fdt=3), ERR_ARG, b"f_dtype must be ADMMQ_DT_F32 or x_dtype"),
    (dict(fdt=DT_F16), ERR_ARG, b"f_dtype"),                               # x is bfloat16
    (dict(codes=0x1004), ERR_ARG, b"16-byte"),
    (dict(x=0x10001), ERR_ARG, b"x must be aligned"),
    (dict(y=0x20002, ydt=DT_F32), ERR_ARG, b"y must be aligned"),
    (dict(bias=0x30002), ERR_ARG, b"bias"),
    (dict(L=0x40002), ERR_ARG, b"L and Rt must be aligned"),
    (dict(Rt=0x50001, fdt=DT_BF16), ERR_ARG, b"L and Rt must be aligned"),
    (dict(M=1 << 30), ERR_ARG, b"range"),
    (dict(K=(1 << 24) + 1), ERR_ARG, b"range"),
    (dict(ws_bytes=4 * 4 * 32 - 1), ERR_WORKSPACE, b"workspace"),          # t alone: 4 nsd N rp bytes, never empty
    (dict(ws=0), ERR_WORKSPACE, b"workspace"),
    (dict(ws=0x100002), ERR_ARG, b"workspace must be float aligned"),
    (dict(ws=0x100004), ERR_ARG, b"workspace must be 16-byte aligned"),
    # parallel regime, tensor_minmax: np + 1 images of [N, M], np N column sums, then t
    (dict(meta=(MINMAX, 4), K=134, ws_bytes=4 * (4 * 4 * 8 + 3 * 4 + 3 * 4 * 32) - 1), ERR_WORKSPACE, b"workspace"),
])
def test_packed_hlrgemm_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    assert _call(lib, **kw) == status
    err = lib.admmq_last_error()
    assert word in err
    if status == ERR_ARG:
        assert b"packed_hlrgemm" in err


def test_plan_and_workspace_queries_are_pure_and_follow_the_plan(lib):
    """np and the regime are admmq_packed_hgemm's; nsd = ranges of 32 ceil(ceil(K / want) / 32) k with
    want = min(ceil(256 / (ceil(r / 64) ceil(N / 64))), 8, ceil(K / 64)); bytes = the y images and column sums of the
    parallel regime rounded up to 16, then 4 nsd N rp."""
    size, plan = lib.admmq_packed_hlrgemm_workspace_size, lib.admmq_packed_hlrgemm_plan
    m, mx = _meta(MSE, 4), _meta(MINMAX, 8)
    for (M, K, N, r), (np_, par, nsd) in NAMED.items():
        out = (ctypes.c_int32 * 4)()
        assert plan(ctypes.byref(m), M, K, N, r, out) == 0 and tuple(out) == (np_, par, nsd, 3 if par else 2), (M, K, N, r, tuple(out))
        assert (par == 1) == (lib.admmq_packed_hgemm_workspace_size(ctypes.byref(m), M, K, N, 1) > 0)
        want = -(-K // min(-(-256 // (-(-r // 64) * -(-N // 64))), 8, -(-K // 64)))
        assert nsd == -(-K // (32 * -(-want // 32)))
        img, t = 4 * (np_ + 1) * N * M * par, 4 * nsd * N * 32 * -(-r // 32)
        assert size(ctypes.byref(m), M, K, N, r) == -(-img // 16) * 16 + t == size(ctypes.byref(m), M, K, N, r)
        assert size(ctypes.byref(mx), M, K, N, r) == -(-(img + 4 * np_ * N * par) // 16) * 16 + t
    out = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    for args in [(0, 64, 4, 8), (8, 0, 4, 8), (8, 64, 0, 8), (8, 64, 4, 0), (8, 64, 4, 257), ((1 << 22) + 1, 65, 1, 8),
                 (8, (1 << 24) + 1, 4, 8)]:
        assert size(ctypes.byref(m), *args) == 0, args
        assert plan(ctypes.byref(m), *args, out) == ERR_ARG and tuple(out) == (7, 7, 7, 7)
    assert size(None, 8, 64, 4, 8) == 0 and plan(None, 8, 64, 4, 8, out) == ERR_ARG
    assert plan(ctypes.byref(m), 8, 64, 4, 8, None) == ERR_ARG


def test_header_declares_what_the_library_exports(lib):
    text = open(os.path.join(ROOT, "include", "admmq.h")).read()
    names = set(re.findall(r"\b(admmq_[a-z0-9_]+)\s*\(", text))
    for n, nargs in (("admmq_packed_hlrgemm", 17), ("admmq_packed_hlrgemm_workspace_size", 5), ("admmq_packed_hlrgemm_plan", 6)):
        assert n in names and hasattr(lib, n)
        proto = re.search(r"\b%s\(([^;]*)\);" % n, text).group(1)
        assert len(proto.split(",")) == nargs == len(getattr(lib, n).argtypes)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_meta_kernel_gives_shapes_and_dtypes(dtype):
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=m)
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)
    L, Rt = torch.empty(64, 5, device=m), torch.empty(5, 134, device=m)
    for out_f32 in (False, True):
        want = torch.float32 if out_f32 else dtype
        y = ops.packed_hlrgemm(codes, words, 64, 134, L, Rt, torch.empty(2, 37, 134, device=m, dtype=dtype), None, out_f32)
        assert tuple(y.shape) == (2, 37, 64) and y.dtype == want
        y = ops.packed_hlrgemm(codes, words, 64, 134, L.to(dtype), Rt.to(dtype), torch.empty(134, device=m, dtype=dtype),
                               torch.empty(64, device=m), out_f32)
        assert tuple(y.shape) == (64,) and y.dtype == want
    x3 = torch.empty(3, 134, device=m, dtype=dtype)
    with pytest.raises(RuntimeError, match="rank r must be 1..256"):
        ops.packed_hlrgemm(codes, words, 64, 134, torch.empty(64, 257, device=m), torch.empty(257, 134, device=m), x3, None, False)
    with pytest.raises(RuntimeError, match="both be float32 or both of x's dtype"):
        ops.packed_hlrgemm(codes, words, 64, 134, L.double(), Rt.double(), x3, None, False)
    with pytest.raises(RuntimeError, match="float16 or bfloat16"):
        ops.packed_hlrgemm(codes, words, 64, 134, L, Rt, x3.float(), None, False)


def test_cpu_tensors_raise_and_fused_false_is_todays_call(monkeypatch):
    import admmq
    from admmq import export, packed
    from admmq.packed import _meta_words
    p = admmq.PackedLowRank(q=_host_packed((6, 10)), L=torch.zeros(6, 2), Rt=torch.zeros(2, 10))
    assert "packed_hlrgemm" in packed.__all__ and admmq.packed_hlrgemm is packed.packed_hlrgemm
    lin = export.PackedLowRankLinear(p)
    assert export.PackedLowRankLinear.fused is False and "fused" not in repr(lin)
    lin.fused = True
    assert "fused" not in lin.state_dict() and "fused" not in lin.get_extra_state() and "fused=True" in repr(lin)
    for dtype in (torch.bfloat16, torch.float16):
        x = torch.zeros(9, 10, dtype=dtype)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            admmq.packed_hlrgemm(p.q.codes, _meta_words(p.q), 6, 10, p.L, p.Rt, x)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            admmq.packed_lowrank_linear(x, p, fused=True)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            lin(x)
    # the routing order: skinny at <= 8 rows, then fused on a half x, else packed_lrgemm with its nine arguments unchanged
    calls = []
    for name in ("packed_lrgemm", "packed_lrgemv", "packed_hlrgemm"):
        monkeypatch.setattr(packed, name, lambda *a, name=name: calls.append((name, a)))
    x32, h8, h9, bias = torch.zeros(9, 10), torch.zeros(2, 4, 10).half(), torch.zeros(9, 10).bfloat16(), torch.zeros(6)
    packed.packed_lowrank_linear(h9, p, bias, torch.float32)
    packed.packed_lowrank_linear(h9, p, bias, None, skinny=True, fused=False)
    packed.packed_lowrank_linear(x32, p, bias, None, fused=True)
    packed.packed_lowrank_linear(h9, p, bias, torch.float32, skinny=True, fused=True)
    packed.packed_lowrank_linear(h8, p, bias, None, fused=True)
    packed.packed_lowrank_linear(h8, p, bias, None, skinny=True, fused=True)
    assert [c[0] for c in calls] == ["packed_lrgemm"] * 3 + ["packed_hlrgemm"] * 2 + ["packed_lrgemv"]
    for (_, a), x, od in zip(calls, (h9, h9, x32, h9, h8, h8), (torch.float32, None, None, torch.float32, None, None)):
        assert len(a) == 9 and a[0] is p.q.codes and a[2:4] == (6, 10) and a[4] is p.L and a[5] is p.Rt
        assert a[6] is x and a[7] is bias and a[8] is od
