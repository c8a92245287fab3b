"""Packed codes, host side (no GPU): the meta record's layout, admmq_packed_bytes, the
argument checks of admmq_quantize_packed (each fails before any device call, with its
documented status and a message), and the Python wrappers' exceptions."""
import ctypes

import pytest
import torch

ERR_ARG, ERR_WORKSPACE, ERR_SCHEME = -1, -3, -4
MSE, MINMAX, SYMMETRIC, AFFINE = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    return _lib.load()


def test_qmeta_is_32_bytes():
    from admmq import _lib
    assert ctypes.sizeof(_lib.QMeta) == 32
    assert [f[0] for f in _lib.QMeta._fields_] == ["scheme", "bits", "scale", "zero_point", "mn", "rng", "index", "bad"]
    assert _lib.QMeta.bad.offset == 28 and _lib.QMeta.scale.offset == 8


@pytest.mark.parametrize("numel,bits,expect", [(1, 1, 1), (7, 3, 3), (8, 3, 3), (9, 3, 4), (1206, 4, 603),
                                               (5, 0, 0), (5, 9, 0), (0, 4, 0), (-3, 4, 0)])
def test_packed_bytes(lib, numel, bits, expect):
    assert lib.admmq_packed_bytes(numel, bits) == expect
    if expect:
        from admmq.packed import packed_bytes
        assert packed_bytes(numel, bits) == expect


def _call(lib, bits, qscheme, codes="ok", code0=0x1000, ws_bytes=None):
    """admmq_quantize_packed on one (9, 134) tensor with made-up device addresses: every
    case below must be refused before anything is launched."""
    from admmq import _lib
    arr = _lib.qtensor_array([_lib.QTensor(0x10000, 0, 9, 134, 0.0, 0.0, 0, 0)])
    need = lib.admmq_quantize_packed_workspace_size(arr, 1, 200)
    assert need >= lib.admmq_quantize_workspace_size(arr, 1, 200) + 8
    cptr = (ctypes.c_void_p * 1)(code0) if codes == "ok" else None
    return lib.admmq_quantize_packed(arr, cptr, ctypes.c_void_p(0x2000), 1, bits, qscheme, 200,
                                     ctypes.c_void_p(0x100000), need if ws_bytes is None else ws_bytes, None)


@pytest.mark.parametrize("kw,status,word", [
    (dict(bits=9, qscheme=MSE), ERR_ARG, b"bits"),
    (dict(bits=0, qscheme=SYMMETRIC), ERR_ARG, b"bits"),
    (dict(bits=1, qscheme=MINMAX), ERR_ARG, b"1 bit"),
    (dict(bits=4, qscheme=4), ERR_SCHEME, b"qscheme"),
    (dict(bits=4, qscheme=MSE, codes=None), ERR_ARG, b"NULL"),
    (dict(bits=4, qscheme=MSE, code0=0x1004), ERR_ARG, b"aligned"),
    (dict(bits=4, qscheme=MSE, ws_bytes=16), ERR_WORKSPACE, b"workspace"),
])
def test_quantize_packed_argument_errors(lib, kw, status, word):
    assert _call(lib, **kw) == status
    assert word in lib.admmq_last_error()


def test_dequantize_packed_argument_errors(lib):
    c = (ctypes.c_void_p * 1)(0x1004)
    y = (ctypes.c_void_p * 1)(0x4000)
    ne = (ctypes.c_int64 * 1)(12)
    assert lib.admmq_dequantize_packed(c, ctypes.c_void_p(0x2000), y, ne, 1, None) == ERR_ARG
    assert b"aligned" in lib.admmq_last_error()
    assert lib.admmq_dequantize_packed(None, ctypes.c_void_p(0x2000), y, ne, 1, None) == ERR_ARG
    ne[0] = 0
    c[0] = 0x1000
    assert lib.admmq_dequantize_packed(c, ctypes.c_void_p(0x2000), y, ne, 1, None) == ERR_ARG


def test_python_wrappers_raise_before_the_device():
    """CPU tensors: the argument errors come first (a valid call would fail on the device check)."""
    import admmq
    x = [torch.zeros(3, 5)]
    with pytest.raises(ValueError, match="bits"):
        admmq.quantize_packed(x, 9, "tensor_symmetric")
    with pytest.raises(ValueError, match="bits"):
        admmq.quantize_packed(x, 0, "tensor_symmetric")
    with pytest.raises(ValueError, match="1 bit"):
        admmq.quantize_packed(x, 1, "tensor_minmax")
    for qs in ("channel_symmetric", "channel_affine"):
        with pytest.raises(ValueError, match="channel"):
            admmq.quantize_packed(x, 4, qs)
    for qs in ("tensor_log", "bogus"):
        with pytest.raises(NotImplementedError):
            admmq.quantize_packed(x, 4, qs)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.quantize_packed(x, 4, "tensor_symmetric")


def test_save_load_and_levels_on_the_host(tmp_path):
    """The file form and the host unpack need no device: a hand-packed 3-bit stream."""
    import numpy as np
    from admmq import PackedTensor, load_packed, save_packed
    lv = np.array([[0, 1, 2, 3, 4], [5, 6, 7, 0, 3], [1, 1, 6, 2, 7]], dtype=np.uint8)
    bits = np.unpackbits(lv.reshape(-1, 1), axis=1, bitorder="little")[:, :3].reshape(-1)
    codes = torch.from_numpy(np.packbits(bits, bitorder="little"))
    p = PackedTensor(codes=codes, shape=(3, 5), bits=3, qscheme="tensor_affine", scale=0.125, zero_point=-2, mn=0.0,
                     rng=0.0, index=-1)
    assert p.nbytes == 6 and p.numel == 15
    assert np.array_equal(p.levels().numpy(), lv)
    save_packed(str(tmp_path / "one.pt"), p)
    q = load_packed(str(tmp_path / "one.pt"))
    assert torch.equal(q.codes, p.codes) and (q.shape, q.bits, q.qscheme, q.scale, q.zero_point, q.index) == \
        ((3, 5), 3, "tensor_affine", 0.125, -2, -1)
    save_packed(str(tmp_path / "two.pt"), [p, q])
    both = load_packed(str(tmp_path / "two.pt"))
    assert len(both) == 2 and torch.equal(both[1].codes, p.codes)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        p.dequantize()


def test_meta_kernels_give_the_shapes():
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes, meta = ops.quantize_packed([torch.empty(9, 134, device=m), torch.empty(7, device=m)], 3, 0)
    assert [tuple(c.shape) for c in codes] == [(453,), (3,)] and all(c.dtype == torch.uint8 for c in codes)
    assert tuple(meta.shape) == (2, 8) and meta.dtype == torch.int32
    ys = ops.dequantize_packed(codes, meta, [9 * 134, 7])
    assert [tuple(y.shape) for y in ys] == [(1206,), (7,)] and ys[0].dtype == torch.float32
