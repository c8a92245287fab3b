"""Skinny integer quant + low-rank GEMV, host side (no GPU): every refusal of admmq_packed_ilrgemv
comes back with its status and its own text before any device call (made-up device addresses), the plan and
workspace queries are pure and follow the written plan, the header declares what the library exports, the Meta kernel
propagates shape and dtype, and CPU tensors raise."""
import ctypes
import os
import re

import pytest
import torch

from test_packed_hgemm_host import AFFINE, DT_BF16, DT_F16, DT_F32, ERR_ARG, ERR_WORKSPACE, MINMAX, MSE, ROOT, _host_packed, _meta

ERR_SCHEME = -4
# (M, K, r) of tests/test_gpu_packed_ilrgemv.py and of the timing tool -> nsd
NAMED = {(33, 65, 5): 1, (65, 261, 37): 2, (33, 4100, 9): 9, (1, 7, 1): 1, (33, 65, 256): 1, (4096, 4096, 32): 16,
         (11008, 4096, 128): 8, (4096, 11008, 128): 8}


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    return _lib.load()


def _actq(bits=8, on=1):
    from admmq import _lib
    return _lib.ActQ(bits, on, -1.0, 2.0)


def _call(lib, meta="ok", codes=0x1000, L=0x40000, Rt=0x50000, fdt=DT_F32, tdt=DT_BF16, r=8, rho=0x60000, x=0x10001, xq="ok",
          rs=0x70000, M=8, K=8, N=4, bias=0, y=0x20000, yc=0, oq=None, cl=0, ws=0x100000, ws_bytes=1 << 20):
    m = _meta() if meta == "ok" else meta
    q = _actq() if xq == "ok" else xq
    P = ctypes.c_void_p
    return lib.admmq_packed_ilrgemv(P(codes), ctypes.byref(m) if m is not None else None, M, K, P(L), P(Rt), fdt, tdt, r, P(rho),
                                    P(x), ctypes.byref(q) if q is not None else None, P(rs), N, P(bias), P(y), P(yc),
                                    ctypes.byref(oq) if oq is not None else None, P(cl), P(ws), ws_bytes, None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(codes=0), ERR_ARG, b"NULL"), (dict(meta=None), ERR_ARG, b"NULL"), (dict(x=0), ERR_ARG, b"NULL"),
    (dict(xq=None), ERR_ARG, b"NULL"), (dict(rs=0), ERR_ARG, b"NULL"),
    (dict(L=0), ERR_ARG, b"L and Rt must not be NULL"), (dict(Rt=0), ERR_ARG, b"L and Rt must not be NULL"),
    (dict(rho=0), ERR_ARG, b"rho must not be NULL"),
    (dict(y=0), ERR_ARG, b"exactly one of y and y_codes"), (dict(yc=0x30000), ERR_ARG, b"exactly one of y and y_codes"),
    (dict(M=0), ERR_ARG, b"positive"), (dict(K=0), ERR_ARG, b"positive"),
    (dict(N=0), ERR_ARG, b"N must be 1..8"), (dict(N=9), ERR_ARG, b"N must be 1..8"),
    (dict(tdt=DT_F32), ERR_ARG, b"t_dtype must be ADMMQ_DT_BF16 or ADMMQ_DT_F16"), (dict(tdt=3), ERR_ARG, b"t_dtype"),
    (dict(fdt=DT_F16), ERR_ARG, b"f_dtype must be ADMMQ_DT_F32 or t_dtype"), (dict(fdt=3), ERR_ARG, b"f_dtype"),
    (dict(r=0), ERR_ARG, b"rank r must be 1..256"), (dict(r=257), ERR_ARG, b"rank r must be 1..256"),
    (dict(meta=(MSE, 0)), ERR_ARG, b"bits"), (dict(meta=(4, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(MINMAX, 4)), ERR_SCHEME, b"no integer form"), (dict(meta=(AFFINE, 4, 2)), ERR_ARG, b"bad"),
    (dict(meta=(AFFINE, 8, 0, 200)), ERR_ARG, b"outside int8"),
    (dict(K=65537), ERR_ARG, b"K must be at most 65536"),
    (dict(xq=_actq(1)), ERR_ARG, b"x_q must be on with bits 2..8"), (dict(xq=_actq(8, 0)), ERR_ARG, b"x_q must be on"),
    (dict(y=0, yc=0x30000), ERR_ARG, b"a codes output needs out_q"),
    (dict(y=0, yc=0x30000, oq=_actq(9)), ERR_ARG, b"a codes output needs out_q"),
    (dict(oq=_actq(25)), ERR_ARG, b"out_q bits must be 1..24"),
    (dict(codes=0x1004), ERR_ARG, b"codes must be 16-byte aligned"),
    (dict(y=0x20002), ERR_ARG, b"4-byte aligned"), (dict(bias=0x30002), ERR_ARG, b"4-byte aligned"),
    (dict(rs=0x70001), ERR_ARG, b"4-byte aligned"), (dict(rho=0x60002), ERR_ARG, b"4-byte aligned"),
    (dict(y=0, yc=0x30000, oq=_actq(4), cl=0x80002), ERR_ARG, b"4-byte aligned"),
    (dict(L=0x40002), ERR_ARG, b"L and Rt must be aligned"), (dict(Rt=0x50001, fdt=DT_BF16), ERR_ARG, b"L and Rt must be aligned"),
    (dict(M=1 << 30), ERR_ARG, b"range"),
    (dict(ws_bytes=4 * 4 * 8 - 1), ERR_WORKSPACE, b"workspace"),          # U32 alone: 4 nsd N r bytes, never empty
    (dict(ws=0), ERR_WORKSPACE, b"workspace"),
    (dict(ws=0x100002), ERR_ARG, b"workspace must be 4-byte aligned"),
    # the split plan at 4 bits (ns = 5, nsd = 9): U32's images, the uint32 images with Sx, q's image
    (dict(K=4100, ws_bytes=4 * (9 * 4 * 8 + 5 * 4 * 9 + 4 * 8) - 1), ERR_WORKSPACE, b"workspace"),
])
def test_packed_ilrgemv_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    assert _call(lib, **kw) == status
    err = lib.admmq_last_error()
    assert word in err and b"packed_ilrgemv" in err


def test_plan_and_workspace_queries_are_pure_and_follow_the_plan(lib):
    """(ks, ns) are admmq_packed_igemv_plan's on (M, K, bits); nsd = ranges of 256 ceil(ceil(K / want) / 256) k with
    want = min(ceil(256 / ceil(r / 4)), 16, ceil(K / 256)); bytes = 4 nsd N r, plus 4 ns N (M + 1) + 4 N M where ns > 1."""
    size, plan = lib.admmq_packed_ilrgemv_workspace_size, lib.admmq_packed_ilrgemv_plan
    for (M, K, r), nsd in NAMED.items():
        for bits in (1, 4, 8):
            m, out, iv = _meta(bits=bits), (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 3)()
            assert plan(ctypes.byref(m), M, K, r, out) == 0 and lib.admmq_packed_igemv_plan(ctypes.byref(m), 0, M, K, iv) == 0
            assert tuple(out) == (iv[0], iv[1], nsd, 3 if iv[1] > 1 else 2), (M, K, r, bits, tuple(out))
            want = -(-K // min(-(-256 // -(-r // 4)), 16, -(-K // 256)))
            assert nsd == -(-K // (256 * -(-want // 256)))
            for N in (1, 8):
                split = 4 * iv[1] * N * (M + 1) + 4 * N * M if iv[1] > 1 else 0
                assert size(ctypes.byref(m), M, K, N, r) == 4 * nsd * N * r + split == size(ctypes.byref(m), M, K, N, r)
    m, out = _meta(), (ctypes.c_int32 * 4)(7, 7, 7, 7)
    for args in [(0, 64, 4, 8), (8, 0, 4, 8), (8, 64, 0, 8), (8, 64, 9, 8), (8, 64, 4, 0), (8, 64, 4, 257), ((1 << 22) + 1, 65, 1, 8),
                 (8, 65537, 4, 8)]:
        assert size(ctypes.byref(m), *args) == 0, args
        if args[2] in (1, 4):
            assert plan(ctypes.byref(m), args[0], args[1], args[3], out) == ERR_ARG and tuple(out) == (7, 7, 7, 7)
    assert plan(ctypes.byref(m), 8, 64, 8, None) == ERR_ARG and plan(None, 8, 64, 8, out) == ERR_ARG


def test_header_declares_what_the_library_exports(lib):
    text = open(os.path.join(ROOT, "include", "admmq.h")).read()
    names = set(re.findall(r"\b(admmq_[a-z0-9_]+)\s*\(", text))
    for n, nargs in (("admmq_packed_ilrgemv", 22), ("admmq_packed_ilrgemv_workspace_size", 5), ("admmq_packed_ilrgemv_plan", 5)):
        assert n in names and hasattr(lib, n)
        proto = re.search(r"\b%s\(([^;]*)\);" % n, text).group(1)
        assert len(proto.split(",")) == nargs == len(getattr(lib, n).argtypes)


def test_meta_kernel_gives_shapes_and_dtypes():
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=m)
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)
    L, Rt, rho, rs = torch.empty(64, 5, device=m), torch.empty(5, 134, device=m), torch.empty(5, device=m), \
        torch.empty(64, dtype=torch.int32, device=m)
    x = torch.empty(2, 4, 134, dtype=torch.uint8, device=m)
    y, cl = ops.packed_ilrgemv(codes, words, 64, 134, L, Rt, rho, 2, x, 8, -1.0, 2.0, rs, None, 0, 0.0, 0.0, False)
    assert tuple(y.shape) == (2, 4, 64) and y.dtype == torch.float32 and cl.numel() == 0
    y, cl = ops.packed_ilrgemv(codes, words, 64, 134, L.half(), Rt.half(), rho, 1, x, 8, -1.0, 2.0, rs, None, 4, -1.0, 2.0, True)
    assert tuple(y.shape) == (2, 4, 64) and y.dtype == torch.uint8 and tuple(cl.shape) == (1,) and cl.dtype == torch.int32
    with pytest.raises(RuntimeError, match="packed_ilrgemv: x must hold 1..8 rows"):
        ops.packed_ilrgemv(codes, words, 64, 134, L, Rt, rho, 2, torch.empty(9, 134, dtype=torch.uint8, device=m), 8, -1.0, 2.0, rs,
                           None, 0, 0.0, 0.0, False)
    with pytest.raises(RuntimeError, match="packed_ilrgemv: tail_dtype must be"):
        ops.packed_ilrgemv(codes, words, 64, 134, L, Rt, rho, 0, x, 8, -1.0, 2.0, rs, None, 0, 0.0, 0.0, False)


def test_cpu_tensors_raise_and_the_names_are_exported():
    import admmq
    from admmq import export, packed
    p = admmq.PackedLowRank(q=_host_packed((6, 10)), L=torch.zeros(6, 2), Rt=torch.zeros(2, 10))
    assert "packed_ilrgemv" in packed.__all__ and admmq.packed_ilrgemv is packed.packed_ilrgemv
    xq = admmq.QuantizedActivation(torch.zeros(8, 10, dtype=torch.uint8), 8, -1.0, 2.0)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_lowrank_linear_int(xq, p, skinny=True)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_ilrgemv(p.q.codes, packed._meta_words(p.q), 6, 10, p.L, p.Rt, torch.zeros(2), xq, torch.zeros(6, dtype=torch.int32))
    lay = export.build_qlr_layer(p, integer=True, in_act=(8, -1.0, 1.0))
    assert lay.skinny is False and "skinny" not in lay.extra_repr() and "skinny" not in lay.get_extra_state()
    lay.skinny = True
    assert "skinny=True" in lay.extra_repr()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lay(torch.zeros(8, 10))
