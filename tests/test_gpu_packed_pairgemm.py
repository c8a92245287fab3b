"""Fused 2-way packed layers on the GPU: packed_pairgemm against plain numpy float64 on
PackedTensor.dequantize() of both weights, at the smallest shapes that cross the kernel's boundaries.

Exact cases: integer activations and weights whose de-quantization is an integer times a power of two, so every
product and partial sum is exact in float32 and the result must equal the float64 reference bit for bit - also
through both quantizers, restated step by step in np.float32. Random cases: the bound of the written sum order."""
import functools

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

DEV = torch.device("cuda:0")
AFF, MINMAX = "tensor_affine", "tensor_minmax"
ULP = 2.0 ** -23   # one full float32 ulp per operation (the MFMA's internal adds are not documented as RNE)
# Operations on a term's path besides the K adds of stage 1's chain and the R adds of stage 2's (include/admmq.h,
# contract items 1 and 3): 1 (product D1 x) + 1 (product D2 t) + 1 (+ bias) + 1 (the second-order terms of
# (1 + u)^(K + R + 3) - 1 <= (K + R + 4) u for K + R < 2^10). The zero padding adds exact zeros.
C_OPS = 4

# (K, R, M, N, layout, (bits1, bits2), transpose1, scheme): one sweep per axis around BASE, plus the corner
BASE = (70, 33, 65, 63, 0, (3, 5), True, AFF)
CASES = [BASE] + [BASE[:0] + (k,) + BASE[1:] for k in (1, 129)] + [BASE[:1] + (r,) + BASE[2:] for r in (1, 65, 256)] + \
    [BASE[:2] + (m,) + BASE[3:] for m in (1, 130)] + [BASE[:3] + (n,) + BASE[4:] for n in (1, 65)] + \
    [(70, 256, 130, 65) + BASE[4:], BASE[:3] + (37, 1) + BASE[5:], BASE[:3] + (37, 1, (3, 5), False, AFF)] + \
    [BASE[:5] + (b,) + BASE[6:] for b in ((1, 8), (4, 4))] + [BASE[:6] + (False, AFF), BASE[:6] + (True, MINMAX)] + \
    [BASE[:3] + (4097,) + BASE[4:], BASE[:3] + (8193, 1) + BASE[5:]]   # 8192 columns and up: the 64-column tile


@functools.lru_cache(maxsize=None)
def _weight(shape, bits, scheme, exact, seed, rows=None):
    """(PackedTensor, float64 de-quantization) of random levels (rows: only the first rows of them). exact: the table
    is integers times 2^-1 (affine, zero point 1) or integers (minmax: rng = n); else an arbitrary scale / range."""
    from admmq import PackedTensor
    lv = np.random.default_rng(seed).integers(0, 1 << bits, size=shape[0] * shape[1], dtype=np.uint8)
    if rows is not None:
        lv, shape = lv[:rows * shape[1]], (rows, shape[1])
    stream = np.packbits(((lv[:, None] >> np.arange(bits)) & 1).astype(np.uint8).reshape(-1), bitorder="little")
    n = float((1 << bits) - 1)
    zp = 1 if bits > 1 else -1
    p = PackedTensor(codes=torch.from_numpy(stream).to(DEV), shape=tuple(shape), bits=bits, qscheme=scheme,
                     scale=0.5 if exact else 0.0371, zero_point=zp if scheme == AFF else 0,
                     mn=-3.0 if exact else -0.81, rng=n if exact else 1.7, index=-1)
    return p, p.dequantize().cpu().numpy().astype(np.float64)


def _operands(case, exact):
    K, R, M, N, layout, bits, trans, scheme = case
    s1 = AFF if bits[0] == 1 else scheme   # (tensor_minmax has no 1 bit code)
    p1, D1 = _weight((K, R) if trans else (R, K), bits[0], s1, exact, 11)
    p2, D2 = _weight((M, R), bits[1], scheme, exact, 23)
    g = torch.Generator().manual_seed(5)
    shape = (N, K) if layout else (2, K, N, 1)
    x = torch.randint(-2, 3, shape, generator=g).float() if exact else torch.randn(shape, generator=g)
    bias = torch.randint(-8, 9, (M,), generator=g).float() if exact else torch.randn(M, generator=g)
    return p1, p2, (D1.T if trans else D1), D2, x.to(DEV), bias.to(DEV)


def _run(case, p1, p2, x, bias, **kw):
    from admmq import packed_conv1x1_pair, packed_linear_pair
    f = packed_linear_pair if case[4] else packed_conv1x1_pair
    y = f(x, p1, p2, bias, transpose1=case[6], **kw)
    return (y if case[4] else y.flatten(2)).cpu().numpy()


def _ref(case, D1, D2, x, bias, mid=None):
    """float64: (y, the absolute sums the bound is made of), in the output's layout."""
    X = x.cpu().numpy().astype(np.float64)
    if case[4]:
        t, ta = X @ D1.T, np.abs(X) @ np.abs(D1).T
        t = mid(t) if mid else t
        return t @ D2.T + bias, (np.abs(t) if mid else ta) @ np.abs(D2).T + np.abs(bias)
    X = X.reshape(X.shape[0], X.shape[1], -1)
    t, ta = np.einsum("rk,bkn->brn", D1, X), np.einsum("rk,bkn->brn", np.abs(D1), np.abs(X))
    t = mid(t) if mid else t
    b = bias[None, :, None]
    return np.einsum("mr,brn->bmn", D2, t) + b, np.einsum("mr,brn->bmn", np.abs(D2), np.abs(t) if mid else ta) + np.abs(b)


def _fq32(v, bits, lo, hi):
    """min_max_quantize's float32 steps (bits >= 2) on exact values, as np.float32 operations; float64 out."""
    v, mn, rng, n = v.astype(np.float32), np.float32(lo), np.float32(hi) - np.float32(lo), np.float32((1 << bits) - 1)
    qi = np.floor(((v - mn) / rng) * n + np.float32(0.5))
    return ((qi * rng) / n + mn).astype(np.float64)


@pytest.mark.parametrize("quant", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_exact_inputs_give_the_float64_result_bit_for_bit(case, quant):
    p1, p2, D1, D2, x, bias = _operands(case, True)
    mid_act, act = ((8, -512.0, 508.0), (6, -4096.0, 4096.0)) if quant else (None, None)   # mid: a grid of 4s, integers
    y64, mag = _ref(case, D1, D2, x, bias.cpu().numpy().astype(np.float64),
                    (lambda t: _fq32(t, *mid_act)) if quant else None)
    assert mag.max() < 2.0 ** 22   # every product and partial sum is an integer below 2^24, in units of 2^-2 at the least
    want = _fq32(y64, *act) if quant else y64
    got = _run(case, p1, p2, x, bias, mid_act=mid_act, act=act)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))


@pytest.mark.parametrize("case", CASES)
def test_random_inputs_stay_within_the_bound_of_the_sum_order(case):
    p1, p2, D1, D2, x, bias = _operands(case, False)
    y64, mag = _ref(case, D1, D2, x, bias.cpu().numpy().astype(np.float64))
    err = np.abs(_run(case, p1, p2, x, bias).astype(np.float64) - y64)
    bound = ULP * (case[0] + case[1] + C_OPS) * mag
    print(f"{case}: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


def test_an_output_depends_on_its_own_column_and_row_only():
    from admmq import packed_conv1x1_pair
    case = (129, 65, 130, 65, 0, (3, 5), True, AFF)
    p1, p2, _, _, x, bias = _operands(case, False)
    acts = dict(mid_act=(7, -6.0, 6.0), act=(5, -20.0, 20.0))
    full = packed_conv1x1_pair(x, p1, p2, bias, **acts)                                    # N = 65, nb = 2
    alone = packed_conv1x1_pair(x[1:, :, :1].contiguous(), p1, p2, bias, **acts)           # N = 1, nb = 1
    rows = _weight((130, 65), 5, AFF, False, 23, rows=65)[0]                               # D2's first 65 rows
    prefix = packed_conv1x1_pair(x[1:, :, :1].contiguous(), p1, rows, bias[:65], **acts)   # M cut to a prefix
    assert torch.equal(full[1:, :, :1], alone) and torch.equal(alone[:, :65], prefix)


@pytest.mark.parametrize("kind", ["cp2conv", "cpfc"])
def test_fused_builders_against_float64(kind):
    from admmq.export import PackedPair, build_cp2conv_layer, build_cpfc_layer
    K, R, M = 70, 33, 65
    case = (K, R, M, 25, 0 if kind == "cp2conv" else 1, (3, 5), True, AFF)
    pin, pout, D1, D2, _, bias = _operands(case, False)
    g = torch.Generator().manual_seed(9)
    if kind == "cp2conv":
        x = torch.randn(2, K, 9, 9, generator=g).to(DEV)
        seq, xs = build_cp2conv_layer(R, [pout, pin], bias, K, M, 0, 2, fused=True), x[:, :, ::2, ::2].reshape(2, K, 25)
    else:
        x = torch.randn(25, K, generator=g).to(DEV)
        seq, xs = build_cpfc_layer(R, [pout, pin], bias, K, M, fused=True), x
    assert [n for n, _ in seq.named_children()] == ["conv12" if kind == "cp2conv" else "fc12"]
    assert isinstance(seq[0], PackedPair)
    y64, mag = _ref(case, D1, D2, xs, bias.cpu().numpy().astype(np.float64))
    y = seq(x).cpu().numpy().astype(np.float64).reshape(y64.shape)
    assert (np.abs(y - y64) <= ULP * (K + R + C_OPS) * mag).all()
