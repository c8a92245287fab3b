"""Fused 2-way packed layers, host side (no GPU): the plan query is pure and follows the rule the
header states, the refusals come back before any device call and leave `out` untouched, the header declares what the
library exports, the Meta kernel propagates shape and dtype, and the Python layers refuse what they must."""
import ctypes
import os
import re

import pytest
import torch

from test_packed_hgemm_host import ERR_ARG, ROOT, _host_packed

# (M, K, N, nb, R): resnet50's 2-way layers (cout, cin, positions, rank) at batch 1 and 32, the rank limit, one column
NAMED = [(64, 64, 3136, b, 16) for b in (1, 32)] + [(256, 64, 3136, b, 25) for b in (1, 32)] + \
    [(1024, 256, 196, b, 102) for b in (1, 32)] + [(2048, 512, 49, b, 204) for b in (1, 32)] + \
    [(2048, 512, 49, 1, 256), (1000, 512, 1, 1, 128), (130, 70, 65, 2, 33)]


@pytest.fixture(scope="module")
def lib():
    from admmq import _lib
    return _lib.load()


def _rule(M, K, N, nb, R):
    """include/admmq.h "Fused packed pair", the plan."""
    up = lambda a, b: -(-a // b)
    C, tm = nb * N, up(M, 64)
    ntile = 32 if up(C, 64) < 128 else 64
    tn = up(C, ntile)
    mt = up(tm, max(1, min(tm, 256 // tn)))
    ms, Rp = up(tm, mt), 32 * up(R, 32)
    return ntile, ms, 4 * (Rp * (ntile + 1) + max(64 * (Rp + 1) + 64 * (ntile + 1), 64 * 65)), tn * ms


@pytest.mark.parametrize("shape", NAMED)
def test_plan_follows_the_written_rule(lib, shape):
    out = (ctypes.c_int32 * 4)()
    assert lib.admmq_packed_pairgemm_plan(*shape, out) == 0
    assert tuple(out) == _rule(*shape) and out[2] <= 160 * 1024 and out[3] >= 1


@pytest.mark.parametrize("shape,word", [((8, 8, 8, 1, 0), b"R must be 1..256"), ((8, 8, 8, 1, 257), b"R must be 1..256"),
                                        ((0, 8, 8, 1, 8), b"positive")])
def test_plan_refusals_leave_out_untouched(lib, shape, word):
    out = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    assert lib.admmq_packed_pairgemm_plan(*shape, out) == ERR_ARG and tuple(out) == (7, 7, 7, 7)
    assert word in lib.admmq_last_error()
    assert lib.admmq_packed_pairgemm_plan(8, 8, 8, 1, 8, None) == ERR_ARG and b"out must not be NULL" in lib.admmq_last_error()


def test_header_declares_what_the_library_exports(lib):
    text = open(os.path.join(ROOT, "include", "admmq.h")).read()
    for n, nargs in (("admmq_packed_pairgemm", 17), ("admmq_packed_pairgemm_plan", 6)):
        assert hasattr(lib, n)
        proto = re.search(r"\b%s\(([^;]*)\);" % n, text).group(1)
        assert len(proto.split(",")) == nargs == len(getattr(lib, n).argtypes)


def test_meta_kernel_gives_shapes_and_dtypes():
    from admmq import _lib
    ops, m = _lib.ops(), torch.device("meta")
    c1, c2 = torch.empty(70 * 33 // 2, dtype=torch.uint8, device=m), torch.empty(65 * 33 // 2 + 1, dtype=torch.uint8, device=m)
    words = torch.tensor([0, 4, 0, 0, 0, 0, -1, 0], dtype=torch.int32)
    y = ops.packed_pairgemm(c1, words, True, c2, words, 65, 70, 33, torch.empty(2, 70, 5, 7, device=m), 0, None, 0, 0.0, 0.0,
                            4, -1.0, 2.0)
    assert tuple(y.shape) == (2, 65, 5, 7) and y.dtype == torch.float32
    y = ops.packed_pairgemm(c1, words, False, c2, words, 65, 70, 33, torch.empty(3, 4, 70, device=m), 1, None, 0, 0.0, 0.0,
                            0, 0.0, 0.0)
    assert tuple(y.shape) == (3, 4, 65) and y.dtype == torch.float32
    with pytest.raises(RuntimeError, match="R must be 1..256"):
        ops.packed_pairgemm(c1, words, True, c2, words, 65, 70, 257, torch.empty(3, 70, device=m), 1, None, 0, 0.0, 0.0, 0, 0.0, 0.0)


def test_python_refusals_and_names():
    import admmq
    from admmq import export, packed
    for n in ("packed_pairgemm", "packed_linear_pair", "packed_conv1x1_pair"):
        assert n in packed.__all__ and getattr(admmq, n) is getattr(packed, n)
    p1, p2 = _host_packed((10, 6)), _host_packed((12, 6))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_linear_pair(torch.zeros(4, 10), p1, p2)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        admmq.packed_conv1x1_pair(torch.zeros(1, 10, 3, 3), p1, p2, stride=2)
    with pytest.raises(TypeError, match="x must be float32"):
        admmq.packed_linear_pair(torch.zeros(4, 10, dtype=torch.bfloat16), p1, p2)
    with pytest.raises(ValueError, match="do not chain"):
        admmq.packed_linear_pair(torch.zeros(4, 10), p1, _host_packed((12, 7)))
    A, B = torch.zeros(12, 6), torch.zeros(10, 6)
    with pytest.raises(ValueError, match="fused=True needs PackedTensor factors"):
        export.build_cp2conv_layer(6, [A, B], None, 10, 12, 0, 1, fused=True)
    with pytest.raises(ValueError, match="fused=True needs PackedTensor factors"):
        export.build_cpfc_layer(6, [A, B], None, 10, 12, fused=True)
    with pytest.raises(ValueError, match="cannot be combined with integer=True"):
        export.build_cp2conv_layer(6, [p2, p1], None, 10, 12, 0, 1, integer=True, in_act=(8, -1.0, 1.0), fused=True)
    with pytest.raises(ValueError, match="needs padding 0"):
        export.build_cp2conv_layer(6, [p2, p1], None, 10, 12, 1, 1, fused=True)
    with pytest.raises(ValueError, match="needs rank <= 256"):
        export.build_cpfc_layer(257, [_host_packed((12, 257)), _host_packed((10, 257))], None, 10, 12, fused=True)
    seq = export.build_cp2conv_layer(6, [p2, p1], torch.zeros(12), 10, 12, 0, 2, act_quant=[(4, -1.0, 1.0), None], fused=True)
    st = seq.state_dict()
    assert sorted(k for k in st if "extra" not in k) == ["conv12.bias", "conv12.codes1", "conv12.codes2"]
    extra = st["conv12._extra_state"]
    assert extra["mid_act"][0] == 4 and extra["act"] is None and extra["stride"] == [2, 2] and extra["first"]["shape"] == [10, 6]
    fresh = export.build_cp2conv_layer(6, [p2, p1], torch.zeros(12), 10, 12, 0, 1, fused=True)
    fresh.load_state_dict(st)
    assert fresh[0].stride == (2, 2) and fresh[0]._mid_act == seq[0]._mid_act
