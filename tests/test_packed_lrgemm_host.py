"""Packed quant + low-rank GEMM, host side (no GPU): every refusal of
admmq_packed_lrgemm comes back with its documented status before any device call (made-up device
addresses), the workspace query is a function of its arguments, the header and the library agree
on the new exports, the Meta kernel propagates shapes, CPU tensors raise, PackedLowRankLinear
refuses mis-shaped factors and act=, and a PackedLowRank round-trips through its file format."""
import ctypes
import os
import re

import pytest
import torch

OK, ERR_ARG, ERR_WORKSPACE = 0, -1, -3
MSE, MINMAX, SYMMETRIC, AFFINE = 0, 1, 2, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    return _lib.load()


def _meta(scheme=MSE, bits=4, bad=0):
    from admmq import _lib
    return _lib.QMeta(scheme, bits, 0.125, 0, 0.0, 1.0, -1, bad)


def _call(lib, meta="ok", codes=0x1000, L=0x30000, Rt=0x40000, r=4, x=0x10000, y=0x20000, M=8, K=8, N=4, bias=0,
          ws=0x100000, ws_bytes=1 << 20):
    m = _meta() if meta == "ok" else meta
    return lib.admmq_packed_lrgemm(ctypes.c_void_p(codes), ctypes.byref(m) if m is not None else None, M, K,
                                   ctypes.c_void_p(L), ctypes.c_void_p(Rt), r, ctypes.c_void_p(x), N,
                                   ctypes.c_void_p(bias), ctypes.c_void_p(y), ctypes.c_void_p(ws), ws_bytes, None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(L=0), ERR_ARG, b"NULL"),
    (dict(Rt=0), ERR_ARG, b"NULL"),
    (dict(codes=0), ERR_ARG, b"NULL"),
    (dict(x=0), ERR_ARG, b"NULL"),
    (dict(y=0), ERR_ARG, b"NULL"),
    (dict(meta=None), ERR_ARG, b"NULL"),
    (dict(r=0), ERR_ARG, b"rank"),
    (dict(r=257), ERR_ARG, b"rank"),
    (dict(M=0), ERR_ARG, b"positive"),
    (dict(K=-3), ERR_ARG, b"positive"),
    (dict(N=0), ERR_ARG, b"positive"),
    (dict(meta=(MSE, 0)), ERR_ARG, b"bits"),
    (dict(meta=(SYMMETRIC, 9)), ERR_ARG, b"bits"),
    (dict(meta=(4, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(-1, 4)), ERR_ARG, b"scheme"),
    (dict(meta=(MINMAX, 1)), ERR_ARG, b"1 bit"),
    (dict(meta=(AFFINE, 4, 2)), ERR_ARG, b"bad"),
    (dict(codes=0x1004), ERR_ARG, b"16-byte"),
    (dict(L=0x30002), ERR_ARG, b"float aligned"),
    (dict(Rt=0x40001), ERR_ARG, b"float aligned"),
    (dict(bias=0x50002), ERR_ARG, b"float aligned"),
    (dict(M=1 << 30), ERR_ARG, b"range"),
    (dict(M=512, K=1141, N=4, ws_bytes=16), ERR_WORKSPACE, b"workspace"),
    (dict(M=512, K=1141, N=4, ws=0, ws_bytes=1 << 30), ERR_WORKSPACE, b"workspace"),
    # the serial regime still needs the workspace: t lives there
    (dict(M=1024, K=134, N=1024, ws=0, ws_bytes=1 << 30), ERR_WORKSPACE, b"workspace"),
    (dict(M=8, K=8, N=4, ws_bytes=4 * 4 * 4 - 1), ERR_WORKSPACE, b"workspace"),
    (dict(ws=0x100002), ERR_ARG, b"workspace must be float aligned"),
])
def test_packed_lrgemm_refusals(lib, kw, status, word):
    kw = dict(kw)
    if isinstance(kw.get("meta"), tuple):
        kw["meta"] = _meta(*kw["meta"])
    assert _call(lib, **kw) == status
    err = lib.admmq_last_error()
    assert word in err
    if status == ERR_ARG:
        assert err.startswith(b"packed_lrgemm: ")


def _pieces(K):
    kp = max(64, 32 * -(-K // 1024))
    return -(-K // kp)


def _ws_formula(M, K, N, r):
    """The documented plan: np + 1 images of y when the GEMM's pieces run in parallel (more than one piece, fewer
    than 256 tiles), and t: one [N, r] image, or np where the down-projection's pieces run in parallel."""
    if min(M, K, N) <= 0 or not 1 <= r <= 256 or M > 1 << 22 or N > 1 << 30 or K > 1 << 24 or M * K >= 1 << 40:
        return 0
    np_ = _pieces(K)
    tiles = lambda rows: -(-rows // 64) * -(-N // 64)   # noqa: E731
    main = (np_ + 1) * N * M * 4 if np_ > 1 and tiles(M) < 256 else 0
    return main + (np_ if np_ > 1 and tiles(r) < 256 else 1) * N * r * 4


def test_workspace_size_is_a_function_of_its_arguments(lib):
    f = lib.admmq_packed_lrgemm_workspace_size
    g = lib.admmq_packed_gemm_workspace_size
    for bad in [(0, 8, 8, 4), (8, 0, 8, 4), (8, 8, -1, 4), (8, 8, 8, 0), (8, 8, 8, 257), (8, 8, 8, -1), (1 << 40, 8, 8, 4),
                (8, 1 << 40, 8, 4), ((1 << 22) + 1, 65, 1, 1), (8, (1 << 24) + 1, 4, 1), (8, 128, (1 << 30) + 1, 1)]:
        assert f(*bad) == 0, bad
    shapes = [(512, 1141, 4, 8), (64, 134, 5, 8), (33, 65, 70, 1), (134, 64, 1, 33), (1024, 134, 1024, 8),
              (4096, 4096, 512, 64), (4096, 4096, 1, 8), (64, 64, 64 * 64, 256), (64, 65, 64 * 64, 256), (8, 8, 4, 4),
              (1 << 22, 65, 1, 1), (8, 1 << 24, 4, 256)]
    first = [f(*s) for s in shapes]
    assert [f(*s) for s in shapes] == first
    for s, b in zip(shapes, first):
        M, K, N, r = s
        assert b == _ws_formula(*s), s
        assert b >= g(M, K, N, 1) + 4 * r * N, s     # the plain GEMM's images and room for t
    # the regimes, read off the sizes: (512, 1141, 4) runs its 18 pieces in parallel, (1024, 134, 1024) serially
    assert g(512, 1141, 4, 1) > 0 and g(1024, 134, 1024, 1) == 0
    assert f(1024, 134, 1024, 8) == 3 * 1024 * 8 * 4     # only t, as three images (16 tiles: its pieces run in parallel)
    assert f(64, 64, 64 * 64, 256) == 64 * 64 * 256 * 4  # one piece: t itself


def test_header_and_library_agree_on_the_new_exports(lib):
    text = open(os.path.join(ROOT, "include", "admmq.h")).read()
    names = set(re.findall(r"\b(admmq_[a-z0-9_]+)\s*\(", text))
    for n in ("admmq_packed_lrgemm", "admmq_packed_lrgemm_workspace_size"):
        assert n in names and hasattr(lib, n)
    proto = re.search(r"int32_t admmq_packed_lrgemm\(([^;]*)\);", text).group(1)
    args = [a.strip() for a in " ".join(proto.split()).split(",")]
    assert len(args) == 14 == len(lib.admmq_packed_lrgemm.argtypes)
    assert [a.split()[-1].lstrip("*") for a in args] == ["codes", "meta", "M", "K", "L", "Rt", "r", "x", "N", "bias", "y",
                                                         "workspace", "workspace_bytes", "stream"]


def test_meta_kernel_gives_the_shapes():
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=m)
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)
    L, Rt = torch.empty(64, 8, device=m), torch.empty(8, 134, device=m)
    y = ops.packed_lrgemm(codes, words, 64, 134, L, Rt, torch.empty(2, 5, 134, device=m), None)
    assert tuple(y.shape) == (2, 5, 64) and y.dtype == torch.float32
    y = ops.packed_lrgemm(codes, words, 64, 134, L, Rt, torch.empty(134, device=m), torch.empty(64, device=m))
    assert tuple(y.shape) == (64,)
    with pytest.raises(RuntimeError, match="x must be"):
        ops.packed_lrgemm(codes, words, 64, 134, L, Rt, torch.empty(3, 64, device=m), None)
    with pytest.raises(RuntimeError, match="L must be"):
        ops.packed_lrgemm(codes, words, 64, 134, torch.empty(64, 7, device=m), Rt, torch.empty(3, 134, device=m), None)
    with pytest.raises(RuntimeError, match="rank"):
        ops.packed_lrgemm(codes, words, 64, 134, torch.empty(64, 257, device=m), torch.empty(257, 134, device=m),
                          torch.empty(3, 134, device=m), None)


def _host_lowrank(shape=(6, 10), r=2, bits=4):
    from admmq import PackedLowRank, PackedTensor
    from admmq.packed import packed_bytes
    g = torch.Generator().manual_seed(3)
    n = shape[0] * shape[1]
    codes = torch.randint(0, 256, (packed_bytes(n, bits),), dtype=torch.uint8, generator=g)
    q = PackedTensor(codes=codes, shape=tuple(shape), bits=bits, qscheme="tensor_symmetric", scale=0.25, zero_point=0,
                     mn=0.0, rng=0.0, index=-1)
    return PackedLowRank(q=q, L=torch.randn(shape[0], r, generator=g), Rt=torch.randn(r, shape[1], generator=g))


def test_cpu_tensors_raise():
    import admmq
    from admmq import export
    p = _host_lowrank()
    assert p.rank == 2 and p.nbytes == 30 + 4 * 2 * (6 + 10)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_lowrank_linear(torch.zeros(3, 10), p)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        export.build_qlr_layer(p)(torch.zeros(3, 10))


def test_layer_holds_codes_and_factors_and_refuses_misshaped_ones():
    import admmq
    from admmq import export
    p = _host_lowrank((6, 10), r=2, bits=3)
    lin = export.PackedLowRankLinear(p, bias=torch.ones(6))
    assert type(export.build_qlr_layer(p, torch.ones(6))) is export.PackedLowRankLinear
    assert not hasattr(lin, "weight")
    assert (lin.in_features, lin.out_features, lin.rank) == (10, 6, 2)
    assert lin.codes.dtype == torch.uint8 and lin.codes.numel() == p.q.nbytes
    assert tuple(lin.L.shape) == (6, 2) and tuple(lin.Rt.shape) == (2, 10) and not lin.bias.requires_grad
    for t in list(lin.parameters()) + list(lin.buffers()):
        assert not (t.dtype == torch.float32 and t.numel() >= 60)
    sd = lin.state_dict()
    assert set(sd) == {"codes", "L", "Rt", "bias", "_extra_state"}
    assert sd["_extra_state"]["bits"] == 3 and sd["_extra_state"]["shape"] == [6, 10] and sd["_extra_state"]["rank"] == 2
    # state_dict round trip on the host: a fresh module with other contents takes the saved ones
    fresh = export.PackedLowRankLinear(_host_lowrank((6, 10), r=2, bits=3), bias=torch.zeros(6))
    fresh.L.zero_()
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.L, lin.L) and torch.equal(fresh.Rt, lin.Rt) and torch.equal(fresh.codes, lin.codes)
    with pytest.raises((ValueError, RuntimeError)):
        export.PackedLowRankLinear(_host_lowrank((6, 10), r=3, bits=3), bias=torch.zeros(6)).load_state_dict(sd)
    # mis-shaped factors
    for L, Rt in [(torch.zeros(5, 2), p.Rt), (p.L, torch.zeros(2, 9)), (torch.zeros(6, 3), p.Rt), (p.L, torch.zeros(10, 2)),
                  (torch.zeros(6, 0), torch.zeros(0, 10)), (torch.zeros(6, 257), torch.zeros(257, 10))]:
        with pytest.raises(ValueError, match="L must be|rank must be"):
            export.PackedLowRankLinear(admmq.PackedLowRank(q=p.q, L=L, Rt=Rt))
    with pytest.raises(TypeError, match="float32"):
        export.PackedLowRankLinear(admmq.PackedLowRank(q=p.q, L=p.L.double(), Rt=p.Rt))
    with pytest.raises(AssertionError, match="Expected shape"):
        export.PackedLowRankLinear(p, bias=torch.ones(7))
    # no activation quantizer on this layer yet
    with pytest.raises(NotImplementedError, match="act"):
        export.PackedLowRankLinear(p, act=(8, -1.0, 1.0))
    with pytest.raises(NotImplementedError):
        lin.set_activation_quant(8, -1.0, 1.0)


def test_packed_lowrank_round_trips_through_its_file(tmp_path):
    import admmq
    p = _host_lowrank((7, 9), r=3, bits=5)
    path = str(tmp_path / "qr.pt")
    admmq.save_packed_lowrank(path, p)
    d = torch.load(path, map_location="cpu", weights_only=True)
    assert d["format"] == "admmq.packed_lowrank.v1"
    q = admmq.load_packed_lowrank(path)
    assert torch.equal(q.q.codes, p.q.codes) and torch.equal(q.L, p.L) and torch.equal(q.Rt, p.Rt)
    assert (q.q.shape, q.q.bits, q.q.qscheme, q.q.scale, q.q.zero_point, q.q.mn, q.q.rng, q.q.index) == \
        (p.q.shape, p.q.bits, p.q.qscheme, p.q.scale, p.q.zero_point, p.q.mn, p.q.rng, p.q.index)
    assert q.rank == 3 and q.nbytes == p.nbytes
    # a wrong format tag is refused, in both directions
    d["format"] = "admmq.packed.v1"
    torch.save(d, path)
    with pytest.raises(ValueError, match="packed_lowrank.v1"):
        admmq.load_packed_lowrank(path)
    admmq.save_packed(path, p.q)
    with pytest.raises(ValueError, match="packed_lowrank.v1"):
        admmq.load_packed_lowrank(path)
    admmq.save_packed_lowrank(path, p)
    with pytest.raises(ValueError, match="not a packed-tensor file"):
        admmq.load_packed(path)


def test_return_packed_keeps_quantize_packed_refusals():
    """The per-channel schemes and tensor_minmax at 1 bit have no packed form: refused on the host, before the loop."""
    from admmq.lowrank import factorize_lowrank
    W = torch.zeros(8, 8)
    with pytest.raises(ValueError, match="per-channel"):
        factorize_lowrank(W, 4, 2, qscheme="channel_symmetric", return_packed=True)
    with pytest.raises(ValueError, match="1-bit code"):
        factorize_lowrank(W, 1, 2, qscheme="tensor_minmax", return_packed=True)
    with pytest.raises(ValueError, match="bits"):
        factorize_lowrank(W, 9, 2, qscheme="tensor_symmetric", return_packed=True)
