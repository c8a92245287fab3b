"""The refusals of the six packed GEMM wrappers on both of their routes: through
torch.ops.admmq and, with ``_lib.use_ops`` turned off, through ctypes. Every call here is refused
before any launch. The texts are those of the wrappers before they shared a call frame, quirks
included: a shape message raised from packed_hgemm / packed_igemm on the op route says
"packed_gemm:", the ctypes route raises ValueError where the op route raises RuntimeError, and a
call with two faults reports its ``x``.

The weight is a 3-bit 70 x 100 code stream of zeros: nothing is quantized, nothing is launched.
packed_igemm has no requires-grad case: its ``x`` is uint8 and it detaches its bias."""
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

M, K = 70, 100
WORDS = torch.tensor([0, 3, 0x3DCCCCCD, 0, 0, 0, -1, 0], dtype=torch.int32)   # mse-minmax, 3 bits, scale 0.1
Q8 = (8, 0.0, 1.0)
R, V = RuntimeError, ValueError

# wrapper: (x shape, x dtype, index of K in the shape)
X_OF = {"gemm": ((5, K), torch.float32, 1), "hgemm": ((5, K), torch.bfloat16, 1), "lrgemm": ((5, K), torch.float32, 1),
        "igemm": ((5, K), torch.uint8, 1), "dwgemm": ((2, K, 6, 5), torch.float32, 1),
        "idwgemm": ((2, K, 6, 5), torch.uint8, 1)}


def _zeros(shape, dtype=torch.float32, device="cuda:0"):
    return torch.zeros(shape, dtype=dtype, device=device)


def _args(wrapper, case):
    """The arguments of a valid call of ``wrapper`` with the faults of ``case`` put in."""
    from admmq.packed import packed_bytes
    shape, dtype, kdim = X_OF[wrapper]
    a = dict(codes=_zeros(packed_bytes(M * K, 3), torch.uint8), x=_zeros(shape, dtype), bias=_zeros(M),
             L=_zeros((M, 3)), Rt=_zeros((3, K)), taps=_zeros((9, K)), image=_zeros((9, 128), torch.int8),
             rowsums=_zeros(M, torch.int32))
    if case in ("wrong_k", "double"):
        a["x"] = _zeros(shape[:kdim] + (K - 1,) + shape[kdim + 1:], dtype)
    if case in ("bias", "double"):
        a["bias"] = _zeros(M - 1)
    if case == "empty":
        a["x"] = _zeros((0,) + shape[1:], dtype)
    if case == "taps":
        a.update(Rt=_zeros((3, K - 1)), taps=_zeros((8, K)), image=_zeros((8, 128), torch.int8))
    if case == "rowsums":
        a["rowsums"] = _zeros(M - 1, torch.int32)
    if case == "grad":
        a["bias" if wrapper == "idwgemm" else "x"].requires_grad_(True)
    if case == "cpu":
        a["x"] = _zeros(shape, dtype, "cpu")
    return a


def _call(wrapper, a):
    from admmq import packed as P
    if wrapper in ("gemm", "hgemm"):
        return P.packed_gemm(a["codes"], WORDS, False, M, K, a["x"], 1, a["bias"])
    if wrapper == "lrgemm":
        return P.packed_lrgemm(a["codes"], WORDS, M, K, a["L"], a["Rt"], a["x"], a["bias"])
    if wrapper == "igemm":
        return P.packed_igemm(a["codes"], WORDS, False, M, K, P.QuantizedActivation(a["x"], *Q8), a["rowsums"], 1, a["bias"])
    if wrapper == "dwgemm":
        return P.packed_dwgemm(a["codes"], WORDS, M, K, a["x"], a["taps"], 3, 1, 1, a["bias"])
    return P._idwgemm(a["codes"], WORDS, M, K, a["x"], Q8, a["image"], 0.1, (3, 3), (1, 1), (1, 1), a["rowsums"], a["bias"],
                      Q8, (0, 0.0, 0.0), False)


# (wrapper, case): ((type, text) on the op route, (type, text) on the ctypes route)
X_GEMM_OPS = (R, "admmq: packed_gemm: x must be [..., 100], got [5, 99]")
GRAD_GEMM = (R, "admmq: packed_gemm is inference only (no backward through packed weights): call it under "
                "torch.no_grad() or detach x")
CPU_GEMM = (R, "admmq: packed_gemm needs its codes and activations on a ROCm GPU (device 'cuda'); the MI355X path has no "
               "CPU implementation")
X_LR = ((R, "admmq: packed_lrgemm: x must be [..., 100], got [5, 99]"), (V, "packed_lrgemm: x must be [..., 100], got (5, 99)"))
X_IG = (X_GEMM_OPS, (V, "packed_igemm: x must be [..., 100], got (5, 99)"))
X_DW = ((R, "admmq: packed_dwgemm: x must be [n, 100, H, W], got [2, 99, 6, 5]"),
        (V, "packed_dwgemm: x must be [n, 100, H, W], got (2, 99, 6, 5)"))
X_IDW = ((R, "admmq: packed_idwgemm: x must be [n, 100, H, W], got [2, 99, 6, 5]"),
         (V, "packed_idwgemm: x must be [n, 100, H, W], got (2, 99, 6, 5)"))
EXPECT = {
    ("gemm", "wrong_k"): (X_GEMM_OPS, (V, "packed_gemm: x must be [..., 100], got (5, 99)")),
    ("gemm", "double"): (X_GEMM_OPS, (V, "packed_gemm: x must be [..., 100], got (5, 99)")),
    ("gemm", "bias"): ((R, "admmq: packed_gemm: bias must be [70], got [69]"), (V, "packed_gemm: bias must be [70], got (69,)")),
    ("gemm", "empty"): ((R, "admmq: packed_gemm: empty x"), (V, "packed_gemm: empty x")),
    ("gemm", "grad"): (GRAD_GEMM, GRAD_GEMM),
    ("gemm", "cpu"): (CPU_GEMM, CPU_GEMM),
    ("hgemm", "wrong_k"): (X_GEMM_OPS, (V, "packed_gemm: x must be [..., 100], got (5, 99)")),
    ("hgemm", "double"): (X_GEMM_OPS, (V, "packed_gemm: x must be [..., 100], got (5, 99)")),
    ("hgemm", "bias"): ((R, "admmq: packed_hgemm: bias must be [70], got [69]"), (V, "packed_gemm: bias must be [70], got (69,)")),
    ("hgemm", "empty"): ((R, "admmq: packed_hgemm: empty x"), (V, "packed_gemm: empty x")),
    ("hgemm", "grad"): (GRAD_GEMM, GRAD_GEMM),
    ("hgemm", "cpu"): (CPU_GEMM, CPU_GEMM),
    ("lrgemm", "wrong_k"): X_LR,
    ("lrgemm", "double"): X_LR,
    ("lrgemm", "bias"): ((R, "admmq: packed_lrgemm: bias must be [70], got [69]"),
                         (V, "packed_lrgemm: bias must be [70], got (69,)")),
    ("lrgemm", "empty"): ((R, "admmq: packed_lrgemm: empty x"), (V, "packed_lrgemm: empty x")),
    ("lrgemm", "taps"): ((R, "admmq: packed_lrgemm: L must be [70, r] and Rt [r, 100], got [70, 3] and [3, 99]"),
                         (V, "packed_lrgemm: L must be [70, r] and Rt [r, 100], got (70, 3) and (3, 99)")),
    ("lrgemm", "grad"): 2 * ((R, "admmq: packed_lrgemm is inference only (no backward through packed weights): call it "
                                 "under torch.no_grad() or detach x"),),
    ("lrgemm", "cpu"): 2 * ((R, "admmq: packed_lrgemm needs its codes, factors and activations on a ROCm GPU (device "
                                "'cuda'); the MI355X path has no CPU implementation"),),
    ("igemm", "wrong_k"): X_IG,
    ("igemm", "double"): X_IG,
    ("igemm", "bias"): ((R, "admmq: packed_igemm: bias must be [70], got [69]"), (V, "packed_igemm: bias must be [70], got (69,)")),
    ("igemm", "empty"): ((R, "admmq: packed_igemm: empty x"), (V, "packed_igemm: empty x")),
    ("igemm", "rowsums"): ((R, "admmq: packed_igemm: rowsums must be an int32 [70] tensor on the GPU"),
                           (V, "packed_igemm: rowsums must be int32 [70]")),
    ("igemm", "cpu"): 2 * ((R, "admmq: packed_igemm needs its codes and activations on a ROCm GPU (device 'cuda'); the "
                               "MI355X path has no CPU implementation"),),
    ("dwgemm", "wrong_k"): X_DW,
    ("dwgemm", "double"): X_DW,
    ("dwgemm", "bias"): ((R, "admmq: packed_dwgemm: bias must be [70], got [69]"),
                         (V, "packed_dwgemm: bias must be [70], got (69,)")),
    ("dwgemm", "empty"): ((R, "admmq: packed_dwgemm: empty x"), (V, "packed_dwgemm: empty x")),
    ("dwgemm", "taps"): ((R, "admmq: packed_dwgemm: taps must be [9, 100], got [8, 100]"),
                         (V, "packed_dwgemm: taps must be [9, 100], got (8, 100)")),
    ("dwgemm", "grad"): 2 * ((R, "admmq: packed_dwgemm is inference only (no backward through packed weights): call it "
                                 "under torch.no_grad() or detach x"),),
    ("dwgemm", "cpu"): 2 * ((R, "admmq: packed_dwgemm needs its codes, taps and activations on a ROCm GPU (device 'cuda'); "
                                "the MI355X path has no CPU implementation"),),
    ("idwgemm", "wrong_k"): X_IDW,
    ("idwgemm", "double"): X_IDW,
    ("idwgemm", "bias"): ((R, "admmq: packed_idwgemm: bias must be [70], got [69]"),
                          (V, "packed_idwgemm: bias must be [70], got (69,)")),
    ("idwgemm", "empty"): ((R, "admmq: packed_idwgemm: empty x"), (V, "packed_idwgemm: empty x")),
    ("idwgemm", "taps"): ((R, "admmq: packed_idwgemm: taps_i8 must be [9, 128], got [8, 128]"),
                          (V, "packed_idwgemm: the tap image must be int8 [9, 128], got torch.int8 (8, 128)")),
    ("idwgemm", "rowsums"): ((R, "admmq: packed_idwgemm: rowsums must be an int32 [70] tensor on the GPU"),
                             (V, "packed_idwgemm: rowsums must be int32 [70]")),
    ("idwgemm", "grad"): 2 * ((R, "admmq: packed_idwgemm is inference only (no backward through packed weights): call it "
                                  "under torch.no_grad() or detach bias"),),
    ("idwgemm", "cpu"): 2 * ((R, "admmq: packed_idwgemm needs its codes, tap image and activations on a ROCm GPU (device "
                                 "'cuda'); the MI355X path has no CPU implementation"),),
}


@pytest.mark.parametrize("route", ["ops", "ctypes"])
@pytest.mark.parametrize("wrapper,case", sorted(EXPECT))
def test_refusal(wrapper, case, route, monkeypatch):
    from admmq import _lib
    assert _lib.use_ops()
    if route == "ctypes":
        monkeypatch.setattr(_lib, "use_ops", lambda: False)
    kind, text = EXPECT[(wrapper, case)][route == "ctypes"]
    a = _args(wrapper, case)
    with pytest.raises(Exception) as e:
        _call(wrapper, a)
    print(f"{wrapper} {case} {route}: {type(e.value).__name__}: {e.value}")
    assert type(e.value) is kind and str(e.value) == text


def test_every_wrapper_has_the_listed_cases():
    for w in X_OF:
        want = {"wrong_k", "bias", "empty", "cpu", "double"}
        want |= {"gemm": {"grad"}, "hgemm": {"grad"}, "lrgemm": {"grad", "taps"}, "igemm": {"rowsums"},
                 "dwgemm": {"grad", "taps"}, "idwgemm": {"grad", "taps", "rowsums"}}[w]
        assert {c for (ww, c) in EXPECT if ww == w} == want, w
