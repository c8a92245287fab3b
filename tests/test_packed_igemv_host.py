"""Skinny integer GEMV, host side (no GPU): every refusal of admmq_packed_igemv comes back with its
status and its own text before any device call (made-up device addresses), the plan and workspace queries are pure
functions that match the written rule, the header declares what the library exports, the Meta kernel gives shape
and dtype for the three output forms, and CPU tensors raise."""
import ctypes
import os
import re

import pytest
import torch

from test_packed_hgemm_host import AFFINE, ERR_ARG, ERR_WORKSPACE, MINMAX, MSE, ROOT, _host_packed, _meta

ERR_SCHEME = -4


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    return _lib.load()


def _call(lib, meta="ok", codes=0x1000, x=0x10000, xq=(8, 1), rs=0x30000, y=0x20000, yc=0, oq=None, cl=0, M=8, K=8, N=4,
          bias=0, ws=0x100000, ws_bytes=1 << 20, trans=0):
    from admmq import _lib
    m = _meta() if meta == "ok" else meta
    q = None if xq is None else _lib.ActQ(xq[0], xq[1], -1.0, 2.0)
    o = None if oq is None else _lib.ActQ(oq[0], oq[1], -1.0, 2.0)
    return lib.admmq_packed_igemv(ctypes.c_void_p(codes), ctypes.byref(m) if m is not None else None, trans, M, K,
                                  ctypes.c_void_p(x), ctypes.byref(q) if q is not None else None, ctypes.c_void_p(rs), N,
                                  ctypes.c_void_p(bias), ctypes.c_void_p(y), ctypes.c_void_p(yc),
                                  ctypes.byref(o) if o is not None else None, ctypes.c_void_p(cl), ctypes.c_void_p(ws),
                                  ws_bytes, None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(codes=0), ERR_ARG, b"NULL"),
    (dict(meta=None), ERR_ARG, b"NULL"),
    (dict(xq=None), ERR_ARG, b"NULL"),
    (dict(rs=0), ERR_ARG, b"NULL"),
    (dict(y=0), ERR_ARG, b"exactly one"),
    (dict(yc=0x40000, oq=(8, 1)), ERR_ARG, b"exactly one"),
    (dict(M=0), ERR_ARG, b"positive"),
    (dict(N=0), ERR_ARG, b"N must be 1..8"),
    (dict(N=9), ERR_ARG, b"N must be 1..8"),
    (dict(meta=(MINMAX, 4)), ERR_SCHEME, b"tensor_minmax"),
    (dict(meta=(MSE, 0)), ERR_ARG, b"bits"),
    (dict(meta=(AFFINE, 4, 2)), ERR_ARG, b"bad"),
    (dict(meta=(AFFINE, 8, 0, 5)), ERR_ARG, b"int8"),
    (dict(K=65537), ERR_ARG, b"65536"),
    (dict(xq=(1, 1)), ERR_ARG, b"x_q"),
    (dict(xq=(8, 0)), ERR_ARG, b"x_q"),
    (dict(y=0, yc=0x40000), ERR_ARG, b"codes output"),
    (dict(y=0, yc=0x40000, oq=(9, 1)), ERR_ARG, b"codes output"),
    (dict(oq=(25, 1)), ERR_ARG, b"1..24"),
    (dict(trans=2), ERR_ARG, b"trans_w"),
    (dict(codes=0x1004), ERR_ARG, b"16-byte"),
    (dict(y=0x20002), ERR_ARG, b"4-byte"),
    (dict(bias=0x50001), ERR_ARG, b"4-byte"),
    (dict(rs=0x30002), ERR_ARG, b"4-byte"),
    (dict(y=0, yc=0x40000, oq=(8, 1), cl=0x60002), ERR_ARG, b"4-byte"),
    (dict(M=1 << 30), ERR_ARG, b"range"),
    (dict(M=8, K=16384, ws_bytes=16), ERR_WORKSPACE, b"workspace"),
    (dict(M=8, K=16384, ws=0), ERR_WORKSPACE, b"workspace"),
    (dict(M=8, K=16384, ws=0x100002), ERR_ARG, b"uint32 aligned"),
])
def test_packed_igemv_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    assert _call(lib, **kw) == status
    err = lib.admmq_last_error()
    assert word in err and b"packed_igemv" in err


def _rule(trans, M, K, bits):
    """DESIGN.md 2.36's planner rule, restated: (ks, ns)."""
    tile, kmin = (256, 256) if trans else (32, 1024)
    while tile * kmin * bits // 8 < 16384:
        kmin *= 2
    tiles = -(-M // tile)
    want = 1 if tiles >= 256 or (not trans and K <= 4096) else min(-(-512 // tiles), 64, -(-K // kmin))
    ks = kmin * -(-(-(-K // want)) // kmin)
    return ks, -(-K // ks)


def test_plan_and_workspace_queries_are_pure_and_follow_the_rule(lib):
    out = (ctypes.c_int32 * 3)()
    named = {(0, 11008, 4096, 4): (4096, 1), (0, 4096, 4096, 8): (4096, 1), (0, 4096, 11008, 8): (3072, 4), (0, 3, 4097, 4): (1024, 5),
             (0, 3, 4096, 4): (4096, 1), (0, 3, 16387, 2): (2048, 9), (0, 2, 65536, 8): (1024, 64), (1, 5, 257, 4): (256, 2),
             (1, 5, 256, 4): (256, 1), (1, 5, 4099, 1): (512, 9), (1, 256, 512, 8): (256, 2), (1, 4096, 4096, 4): (256, 16),
             (1, 70000, 4096, 4): (4096, 1)}
    for (trans, M, K, bits), (ks, ns) in named.items():
        m = _meta(MSE, bits)
        assert _rule(trans, M, K, bits) == (ks, ns), (trans, M, K, bits)
        for _ in range(2):
            assert lib.admmq_packed_igemv_plan(ctypes.byref(m), trans, M, K, out) == 0
            assert tuple(out) == (ks, ns, 2 if ns > 1 else 1), (trans, M, K, bits)
        for N in (1, 3, 8):
            assert lib.admmq_packed_igemv_workspace_size(ctypes.byref(m), trans, M, K, N) == (4 * ns * N * (M + 1) if ns > 1 else 0)
    m = _meta(MSE, 4)
    for args in [(2, 8, 2048, 4), (0, 0, 2048, 4), (0, 8, 0, 4), (0, 8, 2048, 0), (0, 8, 2048, 9), (0, (1 << 22) + 1, 65, 1),
                 (0, 8, 65537, 4)]:
        assert lib.admmq_packed_igemv_workspace_size(ctypes.byref(m), *args) == 0, args
    assert lib.admmq_packed_igemv_workspace_size(None, 0, 8, 2048, 4) == 0
    out[0] = -7
    assert lib.admmq_packed_igemv_plan(ctypes.byref(m), 0, 8, 65537, out) == ERR_ARG and out[0] == -7


def test_header_declares_what_the_library_exports(lib):
    text = open(os.path.join(ROOT, "include", "admmq.h")).read()
    names = set(re.findall(r"\b(admmq_[a-z0-9_]+)\s*\(", text))
    for n, nargs in (("admmq_packed_igemv", 17), ("admmq_packed_igemv_plan", 5), ("admmq_packed_igemv_workspace_size", 5)):
        assert n in names and hasattr(lib, n)
        proto = re.search(r"\b" + n + r"\(([^;]*)\);", text).group(1)
        assert len(proto.split(",")) == nargs == len(getattr(lib, n).argtypes)


def test_meta_kernel_gives_shapes_and_dtypes():
    from admmq import _lib
    ops, m = _lib.ops(), torch.device("meta")
    codes = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=m)
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)
    x, rs = torch.empty(2, 4, 134, dtype=torch.uint8, device=m), torch.empty(64, dtype=torch.int32, device=m)
    for out_bits, out_codes, dtype in ((0, False, torch.float32), (12, False, torch.float32), (6, True, torch.uint8)):
        y, cl = ops.packed_igemv(codes, words, False, 64, 134, x, 8, -1.0, 2.0, rs, None, out_bits, -1.0, 2.0, out_codes)
        assert tuple(y.shape) == (2, 4, 64) and y.dtype == dtype and cl.dtype == torch.int32 and cl.numel() == int(out_codes)
    with pytest.raises(RuntimeError, match="1..8 rows"):
        ops.packed_igemv(codes, words, False, 64, 134, torch.empty(9, 134, dtype=torch.uint8, device=m), 8, -1.0, 2.0, rs, None,
                         0, 0.0, 0.0, False)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.packed_igemv(codes, words, False, 64, 134, torch.empty(3, 134, device=m), 8, -1.0, 2.0, rs, None, 0, 0.0, 0.0, False)


def test_cpu_tensors_raise():
    import admmq
    from admmq.packed import _meta_words
    p = _host_packed((6, 10))
    assert "packed_igemv" in admmq.packed.__all__
    xq = admmq.QuantizedActivation(torch.zeros(3, 10, dtype=torch.uint8), 8, -1.0, 2.0)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_igemv(p.codes, _meta_words(p), False, 6, 10, xq, torch.zeros(6, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_linear_int(xq, p, skinny=True)
