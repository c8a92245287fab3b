"""CPU tests of the Krylov block step's entry points (admmq_cholqr64, admmq_panel_reorth64;
csrc/ortho_kernels.hip): exported, declared, and every refusal answered on the host before
any launch."""
import ctypes
import os

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "admmq.h")
ERR_ARG = -1
A = ctypes.c_void_p(16)   # a non-null dummy address: every call below is refused before a launch
CAP = 64


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libadmmq.so is not built: run __graft_entry__.build()")
    return _lib.load()


def test_symbols_exported_and_declared(lib):
    from admmq import panel
    text = open(HEADER).read()
    for name in ("admmq_cholqr64", "admmq_panel_reorth64"):
        assert hasattr(lib, name) and name + "(" in text
    assert f"#define ADMMQ_CHOLQR_K_MAX {CAP}" in text and panel.CHOLQR_K_MAX == CAP


# (Z, ldz, m, k, G, shift_scale, Q, ldq, info, stream)
@pytest.mark.parametrize("args,text", [
    ((None, 8, 8, 8, A, 0.0, A, 8, None, None), b"null"),
    ((A, 8, 8, 8, None, 0.0, A, 8, None, None), b"null"),
    ((A, 8, 8, 8, A, 0.0, None, 8, None, None), b"null"),
    ((A, 8, 0, 8, A, 0.0, A, 8, None, None), b"positive"),
    ((A, 8, 8, 0, A, 0.0, A, 8, None, None), b"positive"),
    ((A, 7, 8, 8, A, 0.0, A, 8, None, None), b"ldz < k"),
    ((A, 8, 8, 8, A, 0.0, A, 7, None, None), b"ldq < k"),
    ((A, 8, 1 << 31, 8, A, 0.0, A, 8, None, None), b"out of range"),
    ((A, CAP + 1, 8, CAP + 1, A, 0.0, A, CAP + 1, None, None), b"ADMMQ_CHOLQR_K_MAX"),
])
def test_cholqr64_refusals(lib, args, text):
    assert lib.admmq_cholqr64(*args) == ERR_ARG
    assert text in lib.admmq_last_error()


# (K, ldk, m, p, C, ldc, Z, ldz, k, Zout, ldo, stream)
@pytest.mark.parametrize("args,text", [
    ((None, 8, 8, 8, A, 4, A, 4, 4, A, 4, None), b"null"),
    ((A, 8, 8, 8, None, 4, A, 4, 4, A, 4, None), b"null"),
    ((A, 8, 8, 8, A, 4, None, 4, 4, A, 4, None), b"null"),
    ((A, 8, 8, 8, A, 4, A, 4, 4, None, 4, None), b"null"),
    ((A, 8, 0, 8, A, 4, A, 4, 4, A, 4, None), b"positive"),
    ((A, 8, 8, 0, A, 4, A, 4, 4, A, 4, None), b"positive"),
    ((A, 8, 8, 8, A, 4, A, 4, 0, A, 4, None), b"positive"),
    ((A, 7, 8, 8, A, 4, A, 4, 4, A, 4, None), b"ldk < p"),
    ((A, 8, 8, 8, A, 3, A, 4, 4, A, 4, None), b"ldc < k"),
    ((A, 8, 8, 8, A, 4, A, 3, 4, A, 4, None), b"ldz < k"),
    ((A, 8, 8, 8, A, 4, A, 4, 4, A, 3, None), b"ldo < k"),
    ((A, 8, 1 << 31, 8, A, 4, A, 4, 4, A, 4, None), b"out of range"),
    ((A, 8193, 9000, 8193, A, 4, A, 4, 4, A, 4, None), b"out of range"),
    ((A, 8, 8, 8, A, CAP + 1, A, CAP + 1, CAP + 1, A, CAP + 1, None), b"ADMMQ_CHOLQR_K_MAX"),
])
def test_panel_reorth64_refusals(lib, args, text):
    assert lib.admmq_panel_reorth64(*args) == ERR_ARG
    assert text in lib.admmq_last_error()


def test_wrappers_refuse_cpu_tensors():
    import torch
    from admmq import panel
    Z = torch.zeros(8, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        panel.cholqr(Z, torch.eye(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        panel.reorth(Z, torch.zeros(4, 4, dtype=torch.float64), Z)
