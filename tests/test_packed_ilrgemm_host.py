"""Integer quant + low-rank GEMM, host side (no GPU): every refusal of admmq_packed_ilrgemm and
admmq_packed_lowrank_factorsums comes back with its status and its own text before any device call (made-up device
addresses), the plan and workspace queries are pure and follow the written plan, the header declares what the
library exports, the Meta kernels propagate shape and dtype, and CPU tensors raise."""
import ctypes
import os
import re

import pytest
import torch

from test_packed_hgemm_host import AFFINE, DT_BF16, DT_F16, DT_F32, ERR_ARG, ERR_WORKSPACE, MINMAX, MSE, ROOT, _host_packed, _meta

ERR_SCHEME = -4
# (M, K, N, r) -> (np, parallel, nsd): the shapes of tests/test_gpu_packed_ilrgemm.py, and the timing tool's
NAMED = {(134, 134, 70, 24): (3, 1, 3), (64, 134, 37, 70): (3, 1, 3), (33, 65, 9, 5): (2, 1, 2), (1, 7, 1, 3): (1, 0, 1),
         (1024, 65, 1024, 9): (2, 0, 2), (4096, 4096, 16, 32): (32, 1, 8), (4096, 4096, 512, 128): (32, 0, 8),
         (11008, 4096, 64, 32): (32, 1, 8), (4096, 11008, 2048, 128): (29, 0, 4)}


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
    return lib.admmq_packed_ilrgemm(P(codes), ctypes.byref(m) if m is not None else None, M, K, P(L), P(Rt), fdt, tdt, r, P(rho),
                                    P(x), ctypes.byref(q) if q is not None else None, P(rs), N, P(bias), P(y), P(yc),
                                    ctypes.byref(oq) if oq is not None else None, P(cl), P(ws), ws_bytes, None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(codes=0), ERR_ARG, b"NULL"), (dict(meta=None), ERR_ARG, b"NULL"), (dict(x=0), ERR_ARG, b"NULL"),
    (dict(xq=None), ERR_ARG, b"NULL"), (dict(rs=0), ERR_ARG, b"NULL"),
    (dict(L=0), ERR_ARG, b"L and Rt must not be NULL"), (dict(Rt=0), ERR_ARG, b"L and Rt must not be NULL"),
    (dict(rho=0), ERR_ARG, b"rho must not be NULL"),
    (dict(y=0), ERR_ARG, b"exactly one of y and y_codes"), (dict(yc=0x30000), ERR_ARG, b"exactly one of y and y_codes"),
    (dict(M=0), ERR_ARG, b"positive"), (dict(K=0), ERR_ARG, b"positive"), (dict(N=0), ERR_ARG, b"positive"),
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
    (dict(ws_bytes=4 * 4 * 32 - 1), ERR_WORKSPACE, b"workspace"),          # U alone: 4 nsd N rp bytes, never empty
    (dict(ws=0), ERR_WORKSPACE, b"workspace"),
    (dict(ws=0x100004), ERR_ARG, b"workspace must be 16-byte aligned"),
    # parallel regime: np int32 images and q's image of [N, M], then U
    (dict(K=134, ws_bytes=4 * (4 * 4 * 8 + 3 * 4 * 32) - 1), ERR_WORKSPACE, b"workspace"),
])
def test_packed_ilrgemm_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    assert _call(lib, **kw) == status
    err = lib.admmq_last_error()
    assert word in err and b"packed_ilrgemm" in err


@pytest.mark.parametrize("kw,word", [
    (dict(Rt=0), b"NULL"), (dict(rho=0), b"NULL"), (dict(tdt=DT_F32), b"t_dtype"), (dict(fdt=DT_F16), b"f_dtype"),
    (dict(r=0), b"rank r"), (dict(r=257), b"rank r"), (dict(K=0), b"K must be 1..65536"), (dict(K=65537), b"K must be 1..65536"),
    (dict(Rt=0x50002), b"Rt must be aligned"), (dict(rho=0x60001), b"rho must be float aligned"),
])
def test_factorsums_refusals(lib, kw, word):
    a = dict(Rt=0x50000, fdt=DT_F32, tdt=DT_BF16, r=8, K=64, rho=0x60000)
    a.update(kw)
    rc = lib.admmq_packed_lowrank_factorsums(ctypes.c_void_p(a["Rt"]), a["fdt"], a["tdt"], a["r"], a["K"], ctypes.c_void_p(a["rho"]), None)
    assert rc == ERR_ARG and word in lib.admmq_last_error() and b"packed_lowrank_factorsums" in lib.admmq_last_error()


def test_plan_and_workspace_queries_are_pure_and_follow_the_plan(lib):
    """np and the regime are admmq_packed_igemm's; nsd = ranges of 32 ceil(ceil(K / want) / 32) k with
    want = min(ceil(256 / (ceil(r / 64) ceil(N / 64))), 8, ceil(K / 64)); bytes = np int32 images and q's image in the
    parallel regime rounded up to 16, then 4 nsd N rp."""
    size, plan = lib.admmq_packed_ilrgemm_workspace_size, lib.admmq_packed_ilrgemm_plan
    for (M, K, N, r), (np_, par, nsd) in NAMED.items():
        out = (ctypes.c_int32 * 4)()
        assert plan(M, K, N, r, out) == 0 and tuple(out) == (np_, par, nsd, 3 if par else 2), (M, K, N, r, tuple(out))
        assert lib.admmq_packed_igemm_workspace_size(M, K, N, 1) == 4 * np_ * N * M * par
        want = -(-K // min(-(-256 // (-(-r // 64) * -(-N // 64))), 8, -(-K // 64)))
        assert nsd == -(-K // (32 * -(-want // 32)))
        img, u = 4 * (np_ + 1) * N * M * par, 4 * nsd * N * 32 * -(-r // 32)
        assert size(M, K, N, r) == -(-img // 16) * 16 + u == size(M, K, N, r)
    out = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    for args in [(0, 64, 4, 8), (8, 0, 4, 8), (8, 64, 0, 8), (8, 64, 4, 0), (8, 64, 4, 257), ((1 << 22) + 1, 65, 1, 8), (8, 65537, 4, 8)]:
        assert size(*args) == 0, args
        assert plan(*args, out) == ERR_ARG and tuple(out) == (7, 7, 7, 7)
    assert plan(8, 64, 4, 8, None) == ERR_ARG


def test_header_declares_what_the_library_exports(lib):
    text = open(os.path.join(ROOT, "include", "admmq.h")).read()
    names = set(re.findall(r"\b(admmq_[a-z0-9_]+)\s*\(", text))
    for n, nargs in (("admmq_packed_ilrgemm", 22), ("admmq_packed_ilrgemm_workspace_size", 4), ("admmq_packed_ilrgemm_plan", 5),
                     ("admmq_packed_lowrank_factorsums", 7)):
        assert n in names and hasattr(lib, n)
        proto = re.search(r"\b%s\(([^;]*)\);" % n, text).group(1)
        assert len(proto.split(",")) == nargs == len(getattr(lib, n).argtypes)


def test_meta_kernels_give_shapes_and_dtypes():
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=m)
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)
    L, Rt, rho, rs = torch.empty(64, 5, device=m), torch.empty(5, 134, device=m), torch.empty(5, device=m), \
        torch.empty(64, dtype=torch.int32, device=m)
    x = torch.empty(2, 37, 134, dtype=torch.uint8, device=m)
    assert tuple(ops.packed_lowrank_factorsums(Rt.half(), 1).shape) == (5,) and ops.packed_lowrank_factorsums(Rt, 2).dtype == torch.float32
    y, cl = ops.packed_ilrgemm(codes, words, 64, 134, L, Rt, rho, 2, x, 8, -1.0, 2.0, rs, None, 0, 0.0, 0.0, False)
    assert tuple(y.shape) == (2, 37, 64) and y.dtype == torch.float32 and cl.numel() == 0
    y, cl = ops.packed_ilrgemm(codes, words, 64, 134, L.half(), Rt.half(), rho, 1, x, 8, -1.0, 2.0, rs, None, 4, -1.0, 2.0, True)
    assert tuple(y.shape) == (2, 37, 64) and y.dtype == torch.uint8 and tuple(cl.shape) == (1,) and cl.dtype == torch.int32
    with pytest.raises(RuntimeError, match="tail_dtype must be"):
        ops.packed_ilrgemm(codes, words, 64, 134, L, Rt, rho, 0, x, 8, -1.0, 2.0, rs, None, 0, 0.0, 0.0, False)
    with pytest.raises(RuntimeError, match="float32 or of the tail type"):
        ops.packed_ilrgemm(codes, words, 64, 134, L.half(), Rt.half(), rho, 2, x, 8, -1.0, 2.0, rs, None, 0, 0.0, 0.0, False)
    with pytest.raises(RuntimeError, match="rank r must be 1..256"):
        ops.packed_ilrgemm(codes, words, 64, 134, torch.empty(64, 257, device=m), torch.empty(257, 134, device=m), rho, 2, x, 8,
                           -1.0, 2.0, rs, None, 0, 0.0, 0.0, False)
    with pytest.raises(RuntimeError, match="uint8 code tensor"):
        ops.packed_ilrgemm(codes, words, 64, 134, L, Rt, rho, 2, x.float(), 8, -1.0, 2.0, rs, None, 0, 0.0, 0.0, False)


def test_cpu_tensors_raise_and_the_names_are_exported():
    import admmq
    from admmq import export, packed
    p = admmq.PackedLowRank(q=_host_packed((6, 10)), L=torch.zeros(6, 2), Rt=torch.zeros(2, 10))
    for n in ("packed_lowrank_factorsums", "packed_ilrgemm", "packed_lowrank_linear_int"):
        assert n in packed.__all__ and getattr(admmq, n) is getattr(packed, n)
    xq = admmq.QuantizedActivation(torch.zeros(9, 10, dtype=torch.uint8), 8, -1.0, 2.0)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_lowrank_factorsums(p, torch.float16)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_lowrank_linear_int(xq, p)
    with pytest.raises(TypeError, match="tail_dtype"):
        admmq.packed_lowrank_linear_int(xq, p, tail_dtype=torch.float32)
    with pytest.raises(ValueError, match="needs in_act"):
        export.build_qlr_layer(p, integer=True)
    lay = export.build_qlr_layer(p, integer=True, in_act=(8, -1.0, 1.0))
    assert isinstance(lay, export.IntegerPackedLowRank) and lay.get_extra_state()["tail_dtype"] == "bfloat16"
    assert type(export.build_qlr_layer(p)) is export.PackedLowRankLinear
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lay(torch.zeros(9, 10))
