"""torch.ops.admmq: the integer route's operators (no GPU): their schemas, the shapes and dtypes
their Meta kernels propagate, the bits and shape refusals a Meta call already makes, and the
inference-only refusal of the Python entry point."""
import pytest
import torch


@pytest.fixture(scope="module")
def ops():
    from admmq import _lib
    return _lib.ops()


WORDS = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)   # mse-minmax, 4 bits
META = torch.device("meta")


def test_schemas(ops):
    assert str(ops.act_encode.default._schema) == \
        "admmq::act_encode(Tensor x, int bits, float mn, float rng) -> (Tensor codes, Tensor clamped)"
    assert str(ops.act_decode.default._schema) == "admmq::act_decode(Tensor codes, int bits, float mn, float rng) -> Tensor"
    assert str(ops.packed_rowsums.default._schema) == \
        "admmq::packed_rowsums(Tensor codes, Tensor meta_words, bool trans_w, int M, int K) -> Tensor"
    assert str(ops.packed_igemm.default._schema) == (
        "admmq::packed_igemm(Tensor codes, Tensor meta_words, bool trans_w, int M, int K, Tensor x, int x_bits, "
        "float x_mn, float x_rng, Tensor rowsums, int x_layout, Tensor? bias, int out_bits, float out_mn, "
        "float out_rng, bool out_codes) -> (Tensor y, Tensor clamped)")


def test_existing_schemas_are_unchanged(ops):
    assert str(ops.packed_gemm_act.default._schema) == (
        "admmq::packed_gemm_act(Tensor codes, Tensor meta_words, bool trans_w, int M, int K, Tensor x, int x_layout, "
        "Tensor? bias, int out_bits, float out_mn, float out_rng) -> Tensor")
    assert str(ops.fixed_quantize.default._schema) == "admmq::fixed_quantize(Tensor x, int bits, float mn, float rng) -> Tensor"


def test_meta_shapes(ops):
    codes, clamped = ops.act_encode(torch.empty(3, 5, 7, device=META), 4, -1.0, 2.0)
    assert tuple(codes.shape) == (3, 5, 7) and codes.dtype == torch.uint8
    assert tuple(clamped.shape) == (1,) and clamped.dtype == torch.int32
    y = ops.act_decode(torch.empty(3, 5, 7, dtype=torch.uint8, device=META), 4, -1.0, 2.0)
    assert tuple(y.shape) == (3, 5, 7) and y.dtype == torch.float32
    wc = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=META)
    A = ops.packed_rowsums(wc, WORDS, False, 64, 134)
    assert tuple(A.shape) == (64,) and A.dtype == torch.int32
    assert tuple(ops.packed_rowsums(wc, WORDS, True, 134, 64).shape) == (134,)
    rs = torch.empty(64, dtype=torch.int32, device=META)
    y, c = ops.packed_igemm(wc, WORDS, False, 64, 134, torch.empty(3, 134, 7, 5, dtype=torch.uint8, device=META), 8, 0.0, 1.0,
                            rs, 0, None, 0, 0.0, 0.0, False)
    assert tuple(y.shape) == (3, 64, 7, 5) and y.dtype == torch.float32 and c.numel() == 0
    y, c = ops.packed_igemm(wc, WORDS, False, 64, 134, torch.empty(2, 5, 134, dtype=torch.uint8, device=META), 8, 0.0, 1.0,
                            rs, 1, torch.empty(64, device=META), 6, -1.0, 2.0, True)
    assert tuple(y.shape) == (2, 5, 64) and y.dtype == torch.uint8 and tuple(c.shape) == (1,) and c.dtype == torch.int32
    y, _ = ops.packed_igemm(wc, WORDS, False, 64, 134, torch.empty(5, 134, dtype=torch.uint8, device=META), 8, 0.0, 1.0,
                            rs, 1, None, 12, -1.0, 2.0, False)   # a float output takes the 1..24-bit quantizer
    assert y.dtype == torch.float32


def test_meta_refusals(ops):
    x8 = torch.empty(5, 134, dtype=torch.uint8, device=META)
    wc = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=META)
    rs = torch.empty(64, dtype=torch.int32, device=META)
    for bits in (1, 9, 0):
        with pytest.raises(RuntimeError, match="2..8"):
            ops.act_encode(torch.empty(4, device=META), bits, 0.0, 1.0)
        with pytest.raises(RuntimeError, match="2..8"):
            ops.act_decode(torch.empty(4, dtype=torch.uint8, device=META), bits, 0.0, 1.0)
        with pytest.raises(RuntimeError, match="2..8"):
            ops.packed_igemm(wc, WORDS, False, 64, 134, x8, bits, 0.0, 1.0, rs, 1, None, 0, 0.0, 0.0, False)
    with pytest.raises(RuntimeError, match="2..8"):   # a codes output needs a code quantizer
        ops.packed_igemm(wc, WORDS, False, 64, 134, x8, 8, 0.0, 1.0, rs, 1, None, 12, 0.0, 1.0, True)
    with pytest.raises(RuntimeError, match="x must be"):
        ops.packed_igemm(wc, WORDS, False, 64, 134, torch.empty(5, 133, dtype=torch.uint8, device=META), 8, 0.0, 1.0, rs, 1,
                         None, 0, 0.0, 0.0, False)
    with pytest.raises(RuntimeError, match="positive"):
        ops.packed_rowsums(wc, WORDS, False, 0, 134)


def test_cpu_tensors_have_no_kernel(ops):
    with pytest.raises((RuntimeError, NotImplementedError)):
        ops.act_encode(torch.zeros(4), 8, 0.0, 1.0)
    with pytest.raises((RuntimeError, NotImplementedError)):
        ops.act_decode(torch.zeros(4, dtype=torch.uint8), 8, 0.0, 1.0)


def test_requires_grad_is_refused():
    """The Python entry point refuses an input that requires grad before it looks at the device (the
    op's own refusal needs a GPU tensor and is checked in the GPU suite); under no_grad the next
    refusal is the device's."""
    import admmq
    x = torch.zeros(4, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        admmq.act_encode(x, (8, -1.0, 1.0))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            admmq.act_encode(x, (8, -1.0, 1.0))
