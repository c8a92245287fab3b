"""Packed integer codes on the MI355X (DESIGN.md "Packed codes"): the codes de-quantize to
exactly what quantize_tensor returns (IEEE equality: an integer code has no -0.0, so the
comparisons are torch.equal / np.array_equal, never raw bits), the bit stream has the
documented layout, and the C ABI, both Python routes, the files and the CLI agree."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
from conftest import gpu_available
from oracle import quant_oracle as qo

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MSE, MINMAX, SYM, AFF = "tensor_mseminmax_symmetric", "tensor_minmax", "tensor_symmetric", "tensor_affine"
SCHEMES = [MSE, MINMAX, SYM, AFF]
DEV = torch.device("cuda:0")


def np_pack(levels: np.ndarray, bits: int) -> np.ndarray:
    """The layout's definition: element i in bits [i bits, (i + 1) bits) of a little-endian stream."""
    b = np.unpackbits(levels.reshape(-1, 1).astype(np.uint8), axis=1, bitorder="little")[:, :bits]
    return np.packbits(b.reshape(-1), bitorder="little")


def np_unpack(codes: np.ndarray, numel: int, bits: int) -> np.ndarray:
    b = np.unpackbits(codes, bitorder="little")[:numel * bits].reshape(numel, bits)
    return (b.astype(np.uint16) << np.arange(bits, dtype=np.uint16)).sum(axis=1).astype(np.uint8)


def host_dequant(p) -> np.ndarray:
    """The contract's table in numpy float32, from the host-unpacked levels (independent of k_dequant_pack)."""
    u = p.levels().cpu().numpy().astype(np.int32)
    q = 1 << (p.bits - 1)
    if p.qscheme == MINMAX:
        return (u.astype(np.float32) * np.float32(p.rng)) / np.float32((1 << p.bits) - 1) + np.float32(p.mn)
    if p.qscheme == AFF:
        return ((u - q) - p.zero_point).astype(np.float32) * np.float32(p.scale)
    return (u - q).astype(np.float32) * np.float32(p.scale)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


@pytest.fixture(scope="module")
def f1():
    with open(os.path.join(GOLDEN, "f1_quant.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "f1_quant.npz"))


# ------------------------------------------------------------------------------------ 1
def test_roundtrip_equals_reference_fixtures(f1):
    """Every stored F1 case of the four schemes (bits <= 8, a NaN-free reference output, not
    the all-zero input): the codes de-quantize to the reference's output. The fixture stores
    no argmin, so the MSE index (and its scale) is checked against the CPU oracle's."""
    from admmq import quantize_packed
    meta, ref = f1
    seen = 0
    for case in meta:
        if not case["store"] or case["error"] is not None or case["qscheme"] not in SCHEMES:
            continue
        y_ref = ref[case["id"]]
        if case["bits"] > 8 or np.isnan(y_ref).any() or case["kind"] == "zeros":
            continue
        x = gc.f1_input(case)
        kw = {} if case.get("num_attempts") is None else {"num_attempts": case["num_attempts"]}
        if case["qscheme"] == MINMAX and case["bits"] == 1:   # three output values: rejected by contract
            with pytest.raises(ValueError):
                quantize_packed([_dev(x)], 1, MINMAX)
            continue
        p, = quantize_packed([_dev(x)], case["bits"], case["qscheme"], **kw)
        assert p.bad == 0 and p.shape == x.shape and p.bits == case["bits"] and p.qscheme == case["qscheme"]
        assert p.nbytes == math.ceil(x.size * case["bits"] / 8)
        y = p.dequantize().cpu().numpy()
        assert y.shape == y_ref.shape and np.array_equal(y, y_ref), case["id"]
        lv = p.levels().cpu().numpy()
        assert lv.shape == x.shape and int(lv.max()) < (1 << case["bits"]), case["id"]
        if case["qscheme"] == MSE:
            _, info = qo.quantize_tensor_mse(x, case["bits"], kw.get("num_attempts", 200), return_info=True)
            assert p.index == info["index"] and np.float32(p.scale) == info["scale"], case["id"]
        else:
            assert p.index == -1
        seen += 1
    assert seen >= 80   # 48 randn + the num_attempts variants + the finite edge kinds


# ------------------------------------------------------------------------------------ 2
LAYOUT_SHAPES = [(1,), (7,), (8,), (31,), (32,), (3, 11), (9, 134), (134, 9), (64 * 134 + 5,)]


@pytest.mark.parametrize("bits", range(1, 9))
def test_bit_layout(bits):
    """codes == the numpy packing of levels(); the spare bits of the last byte are 0; the
    de-quantized codes equal quantize_tensor. Sizes around the 32-element run of a thread,
    odd last dimensions (the plan's cols % 4 != 0 copy path) and a tail after a whole unit."""
    from admmq import quantize_packed, quantize_tensor
    for k, shape in enumerate(LAYOUT_SHAPES):
        x = _randn(shape, 100 + k)
        numel = x.numel()
        schemes = [MSE, SYM] + ([AFF, MINMAX] if numel in (33, 64 * 134 + 5) else [])
        for qs in schemes:
            if qs == MINMAX and bits == 1:
                continue
            p, = quantize_packed([x], bits, qs)
            codes = p.codes.cpu().numpy()
            assert codes.dtype == np.uint8 and codes.shape == (math.ceil(numel * bits / 8),)
            lv = p.levels().cpu().numpy()
            assert np.array_equal(lv.reshape(-1), np_unpack(codes, numel, bits)), (shape, qs)
            assert np.array_equal(codes, np_pack(lv, bits)), (shape, qs)
            spare = 8 * codes.size - numel * bits
            assert 0 <= spare < 8 and (spare == 0 or codes[-1] >> (8 - spare) == 0), (shape, qs)
            y = quantize_tensor(x, bits, qs)
            assert torch.equal(p.dequantize(), y), (shape, qs)
            assert np.array_equal(host_dequant(p), y.cpu().numpy()), (shape, qs)


@pytest.mark.parametrize("qs,bits", [(MSE, 3), (MINMAX, 4), (AFF, 8)])
def test_large_launch_takes_4096_element_units(qs, bits):
    """From 1024 units of 4096 elements (kPackMinUnits) the final pass takes those instead of
    1024-element units: (2048, 2049) is 1026 of them, the last ones partial or row pads only;
    a 7-element and a (9, 134) tensor ride in the same launch."""
    from admmq import dequantize_packed, quantize_packed, quantize_batched
    xs = [_randn((2048, 2049), 90), _randn((7,), 91), _randn((9, 134), 92)]
    ps = quantize_packed(xs, bits, qs)
    want = quantize_batched(xs, bits, qs)
    for p, y, w in zip(ps, dequantize_packed(ps), want):
        assert p.bad == 0 and p.nbytes == math.ceil(w.numel() * bits / 8)
        assert torch.equal(y, w)
        assert np.array_equal(host_dequant(p), w.cpu().numpy())
        codes = p.codes.cpu().numpy()
        spare = 8 * codes.size - w.numel() * bits
        assert spare == 0 or codes[-1] >> (8 - spare) == 0
    small = quantize_packed(xs[1:], bits, qs)   # the same tensors through the 1024-element units
    for a, b in zip(ps[1:], small):
        assert torch.equal(a.codes, b.codes) and (a.scale, a.zero_point, a.mn, a.rng) == (b.scale, b.zero_point, b.mn, b.rng)


# ------------------------------------------------------------------------------------ 3
def _cabi_packed(xs, bits, code, ys=None, num_attempts=200):
    """admmq_quantize_packed through ctypes; ys: float32 outputs of the same launch (or None)."""
    from admmq import _lib
    lib = _lib.load()
    items = []
    for i, x in enumerate(xs):
        cols = 1 if x.dim() == 0 else x.shape[-1]
        items.append(_lib.QTensor(x.data_ptr(), ys[i].data_ptr() if ys else 0, x.numel() // cols, cols, 0.0, 0.0, 0, 0))
    arr = _lib.qtensor_array(items)
    codes = [torch.zeros(lib.admmq_packed_bytes(x.numel(), bits), dtype=torch.uint8, device=DEV) for x in xs]
    cptr = (ctypes.c_void_p * len(xs))(*[c.data_ptr() for c in codes])
    meta = torch.zeros((len(xs), 8), dtype=torch.int32, device=DEV)
    nb = lib.admmq_quantize_packed_workspace_size(arr, len(xs), num_attempts)
    assert nb > 0
    ws = _lib.workspace(nb, DEV)
    rc = lib.admmq_quantize_packed(arr, cptr, _lib.ptr(meta), len(xs), bits, code, num_attempts, _lib.ptr(ws), nb,
                                   _lib.stream_handle(DEV))
    _lib.check(rc, "quantize_packed")
    torch.cuda.synchronize()
    return codes, meta


@pytest.mark.parametrize("qs", SCHEMES)
def test_same_launch_writes_codes_and_float32(qs):
    """t[i].y set: y is quantize_batched's output bit for bit, the codes those of the
    codes-only call; also with a y that is only 4-byte aligned."""
    from admmq import _lib, quantize_batched
    xs = [_randn((64, 134), 7, 0.3), _randn((128, 278), 8), _randn((33,), 9)]
    if qs in (MSE, AFF):   # enough 4096-element units for the large-launch form of the final pass
        xs.append(_randn((1024, 4100), 10))
    want = quantize_batched(xs, 4, qs)
    c0, m0 = _cabi_packed(xs, 4, _lib.SCHEMES[qs])
    bufs = [torch.full((x.numel() + 4,), 7.0, device=DEV) for x in xs]
    for off in (0, 1):
        ys = [b[off:off + x.numel()].view(x.shape) for b, x in zip(bufs, xs)]
        assert all(y.data_ptr() % 16 == 4 * off for y in ys)
        c1, m1 = _cabi_packed(xs, 4, _lib.SCHEMES[qs], ys)
        for y, w in zip(ys, want):
            assert torch.equal(y.view(torch.int32), w.view(torch.int32)), (qs, off)
        for a, b in zip(c0, c1):
            assert torch.equal(a, b), (qs, off)
        assert torch.equal(m0, m1) and int(m1[:, 7].max()) == 0
        assert all(float(b[off + x.numel()]) == 7.0 for b, x in zip(bufs, xs))   # nothing past the tensor


# ------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("cols", [134, 136])
@pytest.mark.parametrize("bits", [3, 4])
def test_unaligned_input(cols, bits):
    """x whose data pointer is only 4-byte aligned (the scalar load path): same codes as an aligned copy."""
    from admmq import quantize_packed
    buf = _randn((64 * cols + 8,), 21)
    x = buf[1:1 + 64 * cols].view(64, cols)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    xa = x.clone()
    assert xa.data_ptr() % 16 == 0
    for qs in (MSE, AFF):
        p, = quantize_packed([x], bits, qs)
        q, = quantize_packed([xa], bits, qs)
        assert torch.equal(p.codes, q.codes) and (p.scale, p.zero_point, p.index) == (q.scale, q.zero_point, q.index)


# ------------------------------------------------------------------------------------ 5
BATCH_SHAPES = [(9, 134), (64, 134), (128, 278), (1, 1), (7,), (2, 3, 4)]


@pytest.mark.parametrize("qs,bits", [(MSE, 4), (SYM, 3), (AFF, 5), (MSE, 7)])
def test_batch_equals_single_calls(qs, bits):
    """Six tensors of different sizes in one call ((128, 278) spans several units of every
    launch) equal six single calls; dequantize_packed of the batch equals each .dequantize()."""
    from admmq import dequantize_packed, quantize_packed, quantize_batched
    xs = [_randn(s, 40 + k, 0.5) for k, s in enumerate(BATCH_SHAPES)]
    batch = quantize_packed(xs, bits, qs)
    singles = [quantize_packed([x], bits, qs)[0] for x in xs]
    for b, s in zip(batch, singles):
        assert torch.equal(b.codes, s.codes)
        assert (b.shape, b.bits, b.qscheme, b.scale, b.zero_point, b.mn, b.rng, b.index, b.bad) == \
            (s.shape, s.bits, s.qscheme, s.scale, s.zero_point, s.mn, s.rng, s.index, 0)
    ys = dequantize_packed(batch)
    for y, s, w in zip(ys, singles, quantize_batched(xs, bits, qs)):
        assert y.shape == w.shape and torch.equal(y, s.dequantize()) and torch.equal(y, w)


# ------------------------------------------------------------------------------------ 6
MUST_RAISE = [(k, qs) for k in ("nan", "inf") for qs in SCHEMES] + [("zeros", MSE), ("zeros", MINMAX),
                                                                    ("const", MINMAX), ("one", MINMAX)]


def _edge_case(f1, kind, qs):
    return next(c for c in f1[0] if c["kind"] == kind and c["qscheme"] == qs)


@pytest.mark.parametrize("kind,qs", MUST_RAISE)
def test_nan_results_have_no_packed_form(f1, kind, qs):
    from admmq import quantize_packed
    case = _edge_case(f1, kind, qs)
    x = _dev(gc.f1_input(case))
    with pytest.raises(ValueError, match="tensor 0"):
        quantize_packed([x], case["bits"], qs)
    p, = quantize_packed([x], case["bits"], qs, check=False)
    assert p.bad > 0
    ok = _randn((5, 6), 3)
    with pytest.raises(ValueError, match="tensor 1"):   # the message names the tensor's index
        quantize_packed([ok, x], case["bits"], qs)


@pytest.mark.parametrize("qs", [SYM, AFF])
def test_zeros_with_zero_scale_either_way(f1, qs):
    """scale = 0, y = +-0: bad > 0, or bad == 0 with an equal round-trip."""
    from admmq import quantize_packed, quantize_tensor
    case = _edge_case(f1, "zeros", qs)
    x = _dev(gc.f1_input(case))
    p, = quantize_packed([x], case["bits"], qs, check=False)
    if p.bad == 0:
        assert torch.equal(p.dequantize(), quantize_tensor(x, case["bits"], qs))
    else:
        with pytest.raises(ValueError):
            quantize_packed([x], case["bits"], qs)


# ------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("bits", [2, 4, 8])
def test_affine_with_explicit_range(bits):
    from admmq import quantize_packed, quantize_tensor
    x = _randn((64, 134), 11)
    p, = quantize_packed([x], bits, AFF, tmin=-0.5, tmax=0.75)
    assert p.bad == 0 and np.float32(p.scale) == np.float32(1.25) / np.float32(2 ** bits - 1)
    assert torch.equal(p.dequantize(), quantize_tensor(x, bits, AFF, tmin=-0.5, tmax=0.75))
    q, = quantize_packed([x], bits, AFF)
    assert q.scale != p.scale


# ------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("qs", SCHEMES)
def test_ops_route_equals_ctypes_route(qs, monkeypatch):
    from admmq import _lib
    from admmq.packed import dequantize_packed, quantize_packed, quantize_packed_raw
    xs = [_randn((33, 77), 60), _randn((9, 1141), 61), _randn((5,), 62)]
    assert _lib.use_ops()
    c1, m1 = quantize_packed_raw(xs, 4, qs)
    y1 = dequantize_packed(quantize_packed(xs, 4, qs))
    monkeypatch.setenv("ADMMQ_LIB", _lib.LIB_PATH)   # same library, ctypes route
    assert not _lib.use_ops()
    c2, m2 = quantize_packed_raw(xs, 4, qs)
    y2 = dequantize_packed(quantize_packed(xs, 4, qs))
    assert torch.equal(m1, m2)
    for a, b in zip(c1 + y1, c2 + y2):
        assert torch.equal(a, b)


def test_meta_kernels():
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes, meta = ops.quantize_packed([torch.empty(64, 134, device=m), torch.empty(2, 3, 4, device=m)], 5, 0)
    assert [tuple(c.shape) for c in codes] == [(5360,), (15,)] and tuple(meta.shape) == (2, 8)
    assert codes[0].dtype == torch.uint8 and meta.dtype == torch.int32
    ys = ops.dequantize_packed(codes, meta, [64 * 134, 24])
    assert [tuple(y.shape) for y in ys] == [(8576,), (24,)] and ys[1].dtype == torch.float32


# ------------------------------------------------------------------------------------ 9
def test_save_load_roundtrip(tmp_path):
    from admmq import load_packed, quantize_packed, save_packed
    x = _randn((9, 135), 70)
    p, = quantize_packed([x], 3, MSE)
    save_packed(str(tmp_path / "p.pt"), p)
    q = load_packed(str(tmp_path / "p.pt"), device=DEV)
    assert q.codes.device.type == "cuda" and torch.equal(q.codes, p.codes)
    assert (q.shape, q.bits, q.qscheme, q.scale, q.zero_point, q.mn, q.rng, q.index) == \
        (p.shape, p.bits, p.qscheme, p.scale, p.zero_point, p.mn, p.rng, p.index)
    assert torch.equal(q.dequantize(), p.dequantize())
    assert load_packed(str(tmp_path / "p.pt")).codes.device.type == "cpu"


CLI = ["--model-name", "resnet18", "--layer", "layer1.0.conv1", "--method", "admm", "--init", "random", "--rank", "8",
       "--bits", "4", "--qscheme", MSE, "--max_iter_als", "2", "--max_iter_admm", "3", "--seed", "0"]


def test_cli_save_packed(tmp_path):
    from admmq import load_packed
    from admmq.export import factor_prefix, load_factors
    from admmq.factorize import main
    root = str(tmp_path / "packed")
    factors, factors_q = main(CLI + ["--outdir-root", root, "--save-packed"])
    prefix = factor_prefix(root, 4, MSE, "admm", 0, "layer1.0.conv1", "random", 8)
    got = load_factors(prefix, 3, device=DEV, packed=True)
    for n in range(3):
        assert got[n].shape == factors_q[n].shape and torch.equal(got[n], factors_q[n]), n
    assert load_packed(prefix + "mode_0_packed.pt").nbytes == math.ceil(64 * 8 * 4 / 8)
    plain = load_factors(prefix, 3, device=DEV)   # the float32 files are still written
    assert all(torch.equal(a, b) for a, b in zip(plain, factors))
    root2 = str(tmp_path / "plain")
    main(CLI + ["--outdir-root", root2])
    d = os.path.dirname(factor_prefix(root2, 4, MSE, "admm", 0, "layer1.0.conv1", "random", 8))
    names = os.listdir(d)
    assert any(n.endswith("_mode_0.pt") for n in names) and not any(n.endswith("_packed.pt") for n in names)
