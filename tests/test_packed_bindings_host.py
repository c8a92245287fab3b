"""The call frame of the packed GEMM bindings, without a GPU.

Python: the helpers that the ctypes route of the six wrappers shares are plain functions on tensor
metadata, called here on CPU tensors: the geometry they return and the type and text of each refusal.
Ops: the refusals that the Meta kernels of packed_gemm, packed_hgemm, packed_lrgemm and packed_dwgemm
make, with their full texts as they were before the ops shared their checks."""
import pytest
import torch

from admmq import _lib, packed as P

M, K = 70, 100
WORDS = torch.tensor([0, 3, 0x3DCCCCCD, 0, 0, 0, -1, 0], dtype=torch.int32)   # mse-minmax, 3 bits, scale 0.1
META = torch.device("meta")


def _refused(kind, text, fn, *args):
    with pytest.raises(kind) as e:
        fn(*args)
    assert type(e.value) is kind and str(e.value) == text


# ----------------------------------------------------------------- the Python helpers
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
def test_gemm_geometry(dtype):
    x = torch.zeros(2, K, 3, 5, dtype=dtype)[:, :, :, ::2]   # not contiguous
    oshape, nb, N, xc = P._gemm_geometry("w", x, M, K, 0)
    assert (oshape, nb, N) == ((2, M, 3, 3), 2, 9) and xc.is_contiguous() and torch.equal(xc, x)
    x = torch.zeros(4, 3, K, dtype=dtype)
    oshape, nb, N, xc = P._gemm_geometry("w", x, M, K, 1)
    assert (oshape, nb, N) == ((4, 3, M), 1, 12) and xc is x
    oshape, nb, N, _ = P._gemm_geometry("w", torch.zeros(K, dtype=dtype), M, K, 1)
    assert (oshape, nb, N) == ((M,), 1, 1)


def test_gemm_geometry_refusals():
    g = P._gemm_geometry
    _refused(ValueError, "w: x must be [n, 100, ...], got (2, 99, 3)", g, "w", torch.zeros(2, 99, 3), M, K, 0)
    _refused(ValueError, "w: x must be [n, 100, ...], got (2, 100)", g, "w", torch.zeros(2, 100), M, K, 0)
    _refused(ValueError, "w: x must be [..., 100], got (5, 99)", g, "w", torch.zeros(5, 99), M, K, 1)
    _refused(ValueError, "w: x must be [..., 100], got ()", g, "w", torch.zeros(()), M, K, 1)
    _refused(ValueError, "w: x_layout must be 0 or 1", g, "w", torch.zeros(5, 100), M, K, 2)
    _refused(ValueError, "w: empty x", g, "w", torch.zeros(0, 100), M, K, 1)
    _refused(ValueError, "w: empty x", g, "w", torch.zeros(2, 100, 0), M, K, 0)
    _refused(ValueError, "w: x must be [..., 100], got (0, 99)", g, "w", torch.zeros(0, 99), M, K, 1)   # the shape first


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])   # packed_dwgemm's x, packed_idwgemm's codes
def test_depthwise_geometry(dtype):
    x = torch.zeros(2, K, 6, 5, dtype=dtype)
    assert P._dw_x_shape("w", x, K) is None
    nb, H, W, Ho, Wo, xc = P._dw_geometry("w", x, (3, 3), (1, 1), (1, 1))
    assert (nb, H, W, Ho, Wo) == (2, 6, 5, 6, 5) and xc is x
    assert P._dw_geometry("w", x, (3, 2), (2, 3), (0, 1))[3:5] == (2, 2)
    assert P._dw_geometry("w", x, (7, 7), (1, 1), (0, 0))[3:5] == (1, 1)   # (outside the limits: the C call refuses it)
    assert P._dw_geometry("w", x, (3, 3), (0, 0), (1, 1))[3:5] == (6, 5)
    xs = torch.zeros(2, K, 6, 10, dtype=dtype)[:, :, :, ::2]
    xc = P._dw_geometry("w", xs, (3, 3), (1, 1), (1, 1))[5]
    assert xc.is_contiguous() and tuple(xc.shape) == (2, K, 6, 5)
    _refused(ValueError, "w: x must be [n, 100, H, W], got (2, 99, 6, 5)", P._dw_x_shape, "w", torch.zeros(2, 99, 6, 5, dtype=dtype), K)
    _refused(ValueError, "w: x must be [n, 100, H, W], got (2, 100, 6)", P._dw_x_shape, "w", torch.zeros(2, 100, 6, dtype=dtype), K)
    _refused(ValueError, "w: empty x", P._dw_geometry, "w", torch.zeros(0, K, 6, 5, dtype=dtype), (3, 3), (1, 1), (1, 1))


def test_weight_argument():
    buf = torch.arange(64, dtype=torch.uint8)
    cc, meta = P._weight_arg(buf[16:48], WORDS)
    assert cc.data_ptr() == buf.data_ptr() + 16   # aligned: the view itself
    cc, meta = P._weight_arg(buf[3:35], WORDS)
    assert cc.data_ptr() % 16 == 0 and torch.equal(cc, buf[3:35])
    assert (meta.scheme, meta.bits, meta.zero_point, meta.index, meta.bad) == (0, 3, 0, -1, 0)
    assert meta.scale == torch.tensor(0.1).item()
    cc = P._aligned(torch.arange(64, dtype=torch.int8).reshape(4, 16)[:, 1:9])
    assert cc.is_contiguous() and cc.data_ptr() % 16 == 0 and tuple(cc.shape) == (4, 8)


def test_bias_argument(monkeypatch):
    assert P._bias_arg("w", None, M) is None
    _refused(RuntimeError, "admmq: tensors must live on a ROCm GPU (device 'cuda'); the MI355X path has no CPU implementation",
             P._bias_arg, "w", torch.zeros(M), M)
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)
    b = torch.zeros(2 * M)[::2]
    bc = P._bias_arg("w", b, M)
    assert bc.is_contiguous() and tuple(bc.shape) == (M,)
    _refused(ValueError, "w: bias must be [70], got (69,)", P._bias_arg, "w", torch.zeros(69), M)
    _refused(ValueError, "w: bias must be [70], got (70, 1)", P._bias_arg, "w", torch.zeros(70, 1), M)


def test_device_and_inference_refusals():
    text = "admmq: w needs its codes, taps and activations on a ROCm GPU (device 'cuda'); the MI355X path has no CPU implementation"
    _refused(RuntimeError, text, P._require_gpu, "w", "codes, taps and activations", torch.zeros(3), torch.zeros(3))
    _refused(RuntimeError, text, P._require_gpu, "w", "codes, taps and activations", None, None)   # x need not be a tensor
    x = torch.zeros(3, requires_grad=True)
    _refused(RuntimeError, "admmq: w is inference only (no backward through packed weights): call it under torch.no_grad() "
             "or detach bias", P._inference_only, "w", x, "bias")
    with torch.no_grad():
        assert P._inference_only("w", x, "x") is None
    assert P._inference_only("w", x.detach(), "x") is None


def test_quantizer_records():
    assert P._actq((0, 0.0, 0.0)) is None and P._byref(None) is None
    q = P._actq((6, -1.0, 2.5))
    assert (q.bits, q.on, q.mn, q.rng) == (6, 1, -1.0, 2.5)
    assert P._byref(q) is not None


# ----------------------------------------------------------------- the Meta kernels' refusals
@pytest.fixture(scope="module")
def ops():
    return _lib.ops()


def _e(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device=META)


CODES = _e(P.packed_bytes(M * K, 3), dtype=torch.uint8)
X_LAYOUT = "admmq: packed_gemm: x_layout must be 0 (NCHW) or 1 (linear)"
X_LINEAR = "admmq: packed_gemm: x must be [..., 100], got [5, 99]"
X_NCHW = "admmq: packed_gemm: x must be [n, 100, ...] (NCHW), got [2, 99, 4]"


def test_packed_gemm_meta_refusals(ops):
    for call in (lambda x, layout: ops.packed_gemm(CODES, WORDS, False, M, K, x, layout, None),
                 lambda x, layout: ops.packed_gemm_act(CODES, WORDS, False, M, K, x, layout, None, 4, 0.0, 1.0)):
        _refused(RuntimeError, X_LAYOUT, call, _e(5, K), 2)
        _refused(RuntimeError, X_LINEAR, call, _e(5, 99), 1)
        _refused(RuntimeError, X_NCHW, call, _e(2, 99, 4), 0)
        assert tuple(call(_e(2, K, 4), 0).shape) == (2, M, 4)


def test_packed_hgemm_meta_refusals(ops):
    def call(x, layout):
        return ops.packed_hgemm(CODES, WORDS, False, M, K, x, layout, None, False)
    for dt in (torch.bfloat16, torch.float16):   # the shape messages are packed_gemm's
        _refused(RuntimeError, X_LAYOUT, call, _e(5, K, dtype=dt), 2)
        _refused(RuntimeError, X_LINEAR, call, _e(5, 99, dtype=dt), 1)
        _refused(RuntimeError, X_NCHW, call, _e(2, 99, 4, dtype=dt), 0)
        assert call(_e(5, K, dtype=dt), 1).dtype == dt
    _refused(RuntimeError, "admmq: packed_hgemm: x must be float16 or bfloat16, got Float", call, _e(5, K), 1)


def test_packed_lrgemm_meta_refusals(ops):
    def call(L, Rt, x):
        return ops.packed_lrgemm(CODES, WORDS, M, K, L, Rt, x, None)
    _refused(RuntimeError, "admmq: packed_lrgemm: x must be [..., 100], got [5, 99]", call, _e(M, 3), _e(3, K), _e(5, 99))
    _refused(RuntimeError, "admmq: packed_lrgemm: L must be [70, r] and Rt [r, 100], got [70, 3] and [3, 99]", call,
             _e(M, 3), _e(3, 99), _e(5, K))
    _refused(RuntimeError, "admmq: packed_lrgemm: L must be [70, r] and Rt [r, 100], got [69, 3] and [3, 100]", call,
             _e(69, 3), _e(3, K), _e(5, K))
    _refused(RuntimeError, "admmq: packed_lrgemm: L must be [70, r] and Rt [r, 100], got [70, 3] and [4, 100]", call,
             _e(M, 3), _e(4, K), _e(5, K))
    _refused(RuntimeError, "admmq: packed_lrgemm: rank r must be 1..256, got 0", call, _e(M, 0), _e(0, K), _e(5, K))
    _refused(RuntimeError, "admmq: packed_lrgemm: rank r must be 1..256, got 257", call, _e(M, 257), _e(257, K), _e(5, K))
    assert tuple(call(_e(M, 256), _e(256, K), _e(4, 5, K)).shape) == (4, 5, M)


def test_packed_dwgemm_meta_refusals(ops):
    for call in (lambda x, taps, k, p: ops.packed_dwgemm(CODES, WORDS, M, K, x, taps, k, k, 1, 1, p, p, None),
                 lambda x, taps, k, p: ops.packed_dwgemm_act(CODES, WORDS, M, K, x, taps, k, k, 1, 1, p, p, None, 6, 0.0, 1.0,
                                                             0, 0.0, 0.0)):
        _refused(RuntimeError, "admmq: packed_dwgemm: x must be [n, 100, H, W], got [2, 99, 6, 5]", call, _e(2, 99, 6, 5),
                 _e(9, K), 3, 1)
        _refused(RuntimeError, "admmq: packed_dwgemm: taps must be [9, 100], got [8, 100]", call, _e(2, K, 6, 5), _e(8, K), 3, 1)
        _refused(RuntimeError, "admmq: packed_dwgemm: taps must be [9, 100], got [9, 99]", call, _e(2, K, 6, 5), _e(9, 99), 3, 1)
        _refused(RuntimeError, "admmq: packed_dwgemm: the 5 x 5 window does not fit the padded image of x [2, 100, 2, 5]", call,
                 _e(2, K, 2, 5), _e(25, K), 5, 1)
        assert tuple(call(_e(2, K, 6, 5), _e(9, K), 3, 1).shape) == (2, M, 6, 5)
