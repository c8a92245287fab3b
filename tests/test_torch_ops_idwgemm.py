"""torch.ops.admmq: the integer fused depthwise + 1x1 stage's operators (no GPU): their schemas, the
shapes and dtypes their Meta kernels propagate, the refusals a Meta call already makes, the
inference-only refusal of the Python entry point, and that the call stays opaque under
torch.compile the way packed_igemm's does."""
import pytest
import torch


@pytest.fixture(scope="module")
def ops():
    from admmq import _lib
    return _lib.ops()


WORDS = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)   # mse-minmax, 4 bits
META = torch.device("meta")


def test_schemas(ops):
    assert str(ops.packed_taps_i8.default._schema) == \
        "admmq::packed_taps_i8(Tensor codes, Tensor meta_words, int ntaps, int K) -> Tensor"
    assert str(ops.packed_idwgemm.default._schema) == (
        "admmq::packed_idwgemm(Tensor codes, Tensor meta_words, int M, int K, Tensor x, int x_bits, float x_mn, "
        "float x_rng, Tensor taps_i8, float s_c, int kh, int kw, int sh, int sw, int ph, int pw, Tensor rowsums, "
        "Tensor? bias, int mid_bits, float mid_mn, float mid_rng, int out_bits, float out_mn, float out_rng, "
        "bool out_codes, bool count_mid) -> (Tensor y, Tensor mid_clamped, Tensor clamped)")


def test_existing_schemas_are_unchanged(ops):
    assert str(ops.packed_igemm.default._schema) == (
        "admmq::packed_igemm(Tensor codes, Tensor meta_words, bool trans_w, int M, int K, Tensor x, int x_bits, "
        "float x_mn, float x_rng, Tensor rowsums, int x_layout, Tensor? bias, int out_bits, float out_mn, "
        "float out_rng, bool out_codes) -> (Tensor y, Tensor clamped)")
    assert str(ops.packed_dwgemm_act.default._schema) == (
        "admmq::packed_dwgemm_act(Tensor codes, Tensor meta_words, int M, int K, Tensor x, Tensor taps, int kh, int kw, "
        "int sh, int sw, int ph, int pw, Tensor? bias, int mid_bits, float mid_mn, float mid_rng, int out_bits, "
        "float out_mn, float out_rng) -> Tensor")


def _args(x=None, taps=None, xb=8, mb=6, ob=0, out_codes=False, k=(3, 3), s=(1, 1), p=(1, 1), bias=None, K=134,
          count_mid=True):
    wc = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=META)
    rs = torch.empty(64, dtype=torch.int32, device=META)
    x = torch.empty(3, 134, 7, 5, dtype=torch.uint8, device=META) if x is None else x
    taps = torch.empty(k[0] * k[1], 192, dtype=torch.int8, device=META) if taps is None else taps
    return (wc, WORDS, 64, K, x, xb, 0.0, 1.0, taps, 0.125, k[0], k[1], s[0], s[1], p[0], p[1], rs, bias, mb, -1.0, 2.0, ob,
            -1.0, 2.0, out_codes, count_mid)


def test_meta_shapes(ops):
    img = ops.packed_taps_i8(torch.empty(9 * 134 // 2, dtype=torch.uint8, device=META), WORDS, 9, 134)
    assert tuple(img.shape) == (9, 192) and img.dtype == torch.int8
    assert tuple(ops.packed_taps_i8(torch.empty(32, dtype=torch.uint8, device=META), WORDS, 1, 64).shape) == (1, 64)
    y, mc, c = ops.packed_idwgemm(*_args())
    assert tuple(y.shape) == (3, 64, 7, 5) and y.dtype == torch.float32
    assert tuple(mc.shape) == (1,) and mc.dtype == torch.int32 and c.numel() == 0 and c.dtype == torch.int32
    y, mc, c = ops.packed_idwgemm(*_args(s=(2, 2), ob=6, out_codes=True, bias=torch.empty(64, device=META)))
    assert tuple(y.shape) == (3, 64, 4, 3) and y.dtype == torch.uint8 and tuple(c.shape) == (1,) and tuple(mc.shape) == (1,)
    y, _, c = ops.packed_idwgemm(*_args(k=(7, 1), p=(3, 0), ob=12))   # a float output takes the 1..24-bit quantizer
    assert tuple(y.shape) == (3, 64, 7, 5) and y.dtype == torch.float32 and c.numel() == 0
    y, mc, _ = ops.packed_idwgemm(*_args(k=(3, 3), p=(0, 0), count_mid=False))   # a counter not asked for is empty
    assert tuple(y.shape) == (3, 64, 5, 3) and mc.numel() == 0 and mc.dtype == torch.int32


def test_meta_refusals(ops):
    for bits in (1, 9, 0):
        with pytest.raises(RuntimeError, match="2..8"):
            ops.packed_idwgemm(*_args(xb=bits))
        with pytest.raises(RuntimeError, match="2..8"):
            ops.packed_idwgemm(*_args(mb=bits))       # the mid quantizer is mandatory: 0 is refused too
    with pytest.raises(RuntimeError, match="2..8"):   # a codes output needs a code quantizer
        ops.packed_idwgemm(*_args(ob=12, out_codes=True))
    with pytest.raises(RuntimeError, match="x must be"):
        ops.packed_idwgemm(*_args(x=torch.empty(3, 133, 7, 5, dtype=torch.uint8, device=META)))
    with pytest.raises(RuntimeError, match="taps_i8 must be"):
        ops.packed_idwgemm(*_args(taps=torch.empty(9, 134, dtype=torch.int8, device=META)))
    with pytest.raises(RuntimeError, match="kernel size"):
        ops.packed_idwgemm(*_args(k=(8, 1), taps=torch.empty(8, 192, dtype=torch.int8, device=META)))
    with pytest.raises(RuntimeError, match="stride"):
        ops.packed_idwgemm(*_args(s=(0, 1)))
    with pytest.raises(RuntimeError, match="padding"):
        ops.packed_idwgemm(*_args(p=(3, 1)))
    with pytest.raises(RuntimeError, match="does not fit"):
        ops.packed_idwgemm(*_args(x=torch.empty(3, 134, 2, 2, dtype=torch.uint8, device=META), k=(5, 5)))
    with pytest.raises(RuntimeError, match="1..49"):
        ops.packed_taps_i8(torch.empty(32, dtype=torch.uint8, device=META), WORDS, 50, 64)
    with pytest.raises(RuntimeError, match="positive"):
        ops.packed_taps_i8(torch.empty(32, dtype=torch.uint8, device=META), WORDS, 9, 0)


def test_cpu_tensors_have_no_kernel(ops):
    with pytest.raises((RuntimeError, NotImplementedError)):
        ops.packed_taps_i8(torch.zeros(32, dtype=torch.uint8), WORDS, 1, 64)


def _host_packed(shape, bits=4):
    from admmq import PackedTensor
    from admmq.packed import packed_bytes
    return PackedTensor(codes=torch.zeros(packed_bytes(shape[0] * shape[1], bits), dtype=torch.uint8), shape=tuple(shape),
                        bits=bits, qscheme="tensor_symmetric", scale=0.25, zero_point=0, mn=0.0, rng=1.0, index=-1)


def test_requires_grad_is_refused():
    """The Python entry point refuses a bias that requires grad before it looks at the device (the codes
    cannot require grad; the op's own refusal needs GPU tensors and is checked in the GPU suite); under
    no_grad the next refusal is the device's."""
    import admmq
    from admmq import QuantizedActivation
    p = _host_packed((6, 10))
    xq = QuantizedActivation(torch.zeros(1, 10, 4, 4, dtype=torch.uint8), 8, -1.0, 2.0)
    image = (torch.zeros(9, 64, dtype=torch.int8), 0.25)
    bias = torch.zeros(6, requires_grad=True)
    from admmq import packed as pk
    e = pk._int_plan(p, False, "test")
    e[2] = torch.zeros(6, dtype=torch.int32)   # row sums already there: the call reaches the stage itself
    with pytest.raises(RuntimeError, match="inference only"):
        admmq.packed_depthwise_conv1x1_int(xq, image, p, bias=bias, mid_act=(6, -1.0, 1.0))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            admmq.packed_depthwise_conv1x1_int(xq, image, p, bias=bias, mid_act=(6, -1.0, 1.0))


def test_the_call_is_opaque_under_torch_compile():
    """As packed_igemm's: while the tracer is compiling the call goes through a torch.compiler.disable
    wrapper (the host meta record beside device tensors is not traceable), and the integer layer's
    forward is such a wrapper itself; the compiled layer is run in the GPU suite."""
    from admmq import export, packed as pk
    for f in (pk._opaque_idwgemm, pk._opaque_igemm, pk._taps_i8, export.IntegerPackedCP.forward,
              export.IntegerPackedPair.forward):
        assert getattr(f, "_torchdynamo_disable", False), f
