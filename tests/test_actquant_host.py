"""Fixed-range activation quantizers without a GPU: the exported symbols and the
record's size, every refusal of the three entry points (its status and a text of its own, before
any launch), the workspace rule, the (mn, rng) type rule and the Python-side refusals."""
import ctypes

import numpy as np
import pytest
import torch

ERR_ARG = -1   # ADMMQ_ERR_ARG (include/admmq.h)


def _lib():
    from admmq import _lib
    return _lib


def _err():
    return _lib().load().admmq_last_error().decode()


def test_symbols_and_record_size():
    L = _lib()
    lib = L.load()
    for name in ("admmq_fixed_quantize", "admmq_packed_gemm_act", "admmq_packed_dwgemm_act"):
        assert hasattr(lib, name), name
    assert ctypes.sizeof(L.ActQ) == 16


def test_fixed_quantize_refusals():
    L = _lib()
    lib = L.load()
    buf = (ctypes.c_float * 8)()
    x = ctypes.cast(buf, ctypes.c_void_p)
    on = L.ActQ(4, 1, 0.3, 1.1)
    texts = set()
    for args in [(None, x, 8, ctypes.byref(on)), (x, None, 8, ctypes.byref(on)), (x, x, 8, None),
                 (x, x, 8, ctypes.byref(L.ActQ(4, 0, 0.3, 1.1))), (x, x, 8, ctypes.byref(L.ActQ(0, 1, 0.3, 1.1))),
                 (x, x, 8, ctypes.byref(L.ActQ(25, 1, 0.3, 1.1))), (x, x, 0, ctypes.byref(on)),
                 (x, x, -3, ctypes.byref(on)), (ctypes.c_void_p(x.value + 2), x, 4, ctypes.byref(on))]:
        assert lib.admmq_fixed_quantize(*args, None) == ERR_ARG, args
        texts.add(_err())
    assert len(texts) == 5 and all(t.startswith("fixed_quantize:") for t in texts), texts


def test_packed_act_refusals_and_workspace():
    L = _lib()
    lib = L.load()
    codes = (ctypes.c_uint8 * 4096)()
    c = ctypes.c_void_p((ctypes.addressof(codes) + 15) & ~15)
    f = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    meta = L.QMeta(0, 4, 0.1, 0, 0.0, 0.0, 0, 0)
    bad = L.ActQ(25, 1, 0.0, 1.0)
    off_bad = L.ActQ(99, 0, 0.0, 1.0)   # off: its bits are not looked at
    m = ctypes.byref(meta)
    assert lib.admmq_packed_gemm_act(c, m, 0, 8, 8, f, 0, 4, 1, None, f, ctypes.byref(bad), None, 0, None) == ERR_ARG
    assert _err() == "packed_gemm_act: out_q bits must be 1..24"
    assert lib.admmq_packed_gemm_act(None, m, 0, 8, 8, f, 0, 4, 1, None, f, ctypes.byref(off_bad), None, 0, None) == ERR_ARG
    assert "must not be NULL" in _err()
    dw = lambda mq, oq, ws, wsb, M=8, K=8: lib.admmq_packed_dwgemm_act(c, m, M, K, f, 1, 4, 4, f, 3, 3, 1, 1, 1, 1, None, f,
                                                                         mq, oq, ws, wsb, None)
    assert dw(ctypes.byref(bad), None, None, 0) == ERR_ARG and _err() == "packed_dwgemm_act: mid_q bits must be 1..24"
    assert dw(None, ctypes.byref(bad), None, 0) == ERR_ARG and _err() == "packed_dwgemm_act: out_q bits must be 1..24"
    # the workspace is the parent's: a size one byte short of it is refused as the parent refuses it
    on = L.ActQ(8, 1, 0.0, 1.0)
    need = lib.admmq_packed_gemm_workspace_size(512, 1141, 4, 1)
    assert need > 0 and need == lib.admmq_packed_dwgemm_workspace_size(512, 1141, 2, 2, 1)
    ADMMQ_ERR_WORKSPACE = lib.admmq_packed_gemm(c, m, 0, 512, 1141, f, 0, 4, 1, None, f, f, need - 1, None)
    assert ADMMQ_ERR_WORKSPACE not in (0, ERR_ARG)
    assert lib.admmq_packed_gemm_act(c, m, 0, 512, 1141, f, 0, 4, 1, None, f, ctypes.byref(on), f, need - 1, None) == \
        ADMMQ_ERR_WORKSPACE
    assert lib.admmq_packed_dwgemm_act(c, m, 512, 1141, f, 1, 4, 4, f, 3, 3, 2, 2, 1, 1, None, f, ctypes.byref(on),
                                       ctypes.byref(on), f, need - 1, None) == ADMMQ_ERR_WORKSPACE


def _fixture():
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "f12_actquant.json")) as f:
        return json.load(f)["cases"]


def test_range_rule_reproduces_the_fixture():
    """The (mn, rng) recorded beside the reference's min_max_quantize outputs, for tensor, float and
    both mixed ranges (a tensor bound and a Python number: both float32 first, then a float32 subtraction)."""
    from admmq.quantization import act_range
    seen = set()
    for c in _fixture():
        if c["kind"] != "min_max":
            continue
        lo = torch.tensor(c["min"], dtype=torch.float32) if c["route"] in ("tensor", "mixed_tf") else c["min"]
        hi = torch.tensor(c["max"], dtype=torch.float32) if c["route"] in ("tensor", "mixed_ft") else c["max"]
        assert act_range(lo, hi) == (c["mn"], c["rng"]), c["id"]
        seen.add(c["route"])
    assert seen == {"tensor", "float", "mixed_tf", "mixed_ft"}


def test_range_type_rule():
    """Against torch's own arithmetic on the CPU: (input - min) and (max - min) as the reference writes them."""
    from admmq.quantization import act_range
    g = np.random.default_rng(3)
    one = torch.ones(1, dtype=torch.float32)
    for _ in range(200):
        lo, hi = float(g.normal()), float(g.normal() * 3)
        lo_t, hi_t = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
        for a, b in [(lo, hi), (lo_t, hi_t), (lo_t, hi), (lo, hi_t)]:
            mn, rng = act_range(a, b)
            assert mn == float(lo_t)
            # torch: a float32 tensor times (max - min) rounds a Python difference once, a tensor one in float32
            assert rng == float((one * (b - a))[0]), (a, b)
    assert act_range(0.3, 1.4) == (float(np.float32(0.3)), float(np.float32(1.4 - 0.3)))
    with pytest.raises(ValueError):
        act_range(torch.zeros(2), 1.0)


def test_python_refusals():
    from admmq import fixed_quantize, min_max_quantize
    from admmq.quantization import act_record
    x = torch.zeros(4)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        fixed_quantize(x, 4, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        min_max_quantize(x, 4, 0.0, 1.0)
    for bits in (0, 25):
        with pytest.raises(ValueError):
            act_record(bits, 0.0, 1.0)
    from admmq.packed import packed_gemm
    with pytest.raises(RuntimeError, match="ROCm GPU"):   # CPU tensors are refused as the plain call refuses them
        packed_gemm(torch.zeros(32, dtype=torch.uint8), torch.zeros(8, dtype=torch.int32), False, 8, 8,
                    torch.zeros(1, 8, 2, 2), 0, None, act=(4, 0.0, 1.0))


def test_meta_kernels_give_the_shapes():
    from admmq import _lib
    ops = _lib.ops()
    m = torch.device("meta")
    codes, words = torch.empty(64 * 134 // 2, dtype=torch.uint8, device=m), torch.zeros(8, dtype=torch.int32)
    y = ops.packed_gemm_act(codes, words, False, 64, 134, torch.empty(3, 134, 7, 5, device=m), 0, None, 4, 0.3, 1.1)
    assert y.shape == (3, 64, 7, 5) and y.dtype == torch.float32 and y.device.type == "meta"
    y = ops.packed_gemm_act(codes, words, True, 134, 64, torch.empty(9, 64, device=m), 1, None, 0, 0.0, 0.0)
    assert y.shape == (9, 134)
    y = ops.packed_dwgemm_act(codes, words, 64, 134, torch.empty(2, 134, 9, 8, device=m), torch.empty(9, 134, device=m),
                              3, 3, 2, 2, 1, 1, None, 4, 0.3, 1.1, 8, -1.0, 2.0)
    assert y.shape == (2, 64, 5, 4)
    assert ops.fixed_quantize(torch.empty(3, 5, device=m), 8, 0.0, 1.0).shape == (3, 5)
    with pytest.raises(RuntimeError, match="bits must be 1..24"):
        ops.fixed_quantize(torch.empty(3, device=m), 25, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="bits must be 1..24"):
        ops.packed_gemm_act(codes, words, False, 64, 134, torch.empty(3, 134, 7, 5, device=m), 0, None, 25, 0.3, 1.1)


def test_modules_on_the_cpu():
    from torch import nn
    from admmq import actquant as aq
    q = aq.get_quant_layer("minmax", "conv1", bits=8, counter=6)
    assert type(q) is aq.MinMaxQuant and q.name == "conv1_quant" and q.counter == 6 and q.bits == 8
    assert repr(q) == "MinMaxQuant(bits=8 min_val=None max_val=None)"
    a = aq.get_quant_layer("avgminmax", "s", bits=4, counter=3)
    assert type(a) is aq.MovingAvgMinMaxQuant and a.averaging_constant == 0.01 and a.counter == 3
    f = aq.get_quant_layer("fixed", "s", bits=4, zero_point=0.5, scope=2.0)
    assert repr(f) == "FixedQuant(bits=4 zero_point=0.5 scope=2.0)"
    none = aq.FixedQuant("s", 4, zero_point=None, scope=None)
    x = torch.arange(8.0)
    assert none(x) is x
    # observing is plain torch and runs anywhere; the counter falls by the batch length
    b1, b2 = torch.tensor([[1.0, -2.0], [0.5, 3.0]]), torch.tensor([[5.0, 0.0]])
    assert q(b1) is b1 and q.counter == 4 and float(q.min_val) == -2.0 and float(q.max_val) == 3.0
    assert q(b2) is b2 and q.counter == 3 and float(q.min_val) == -2.0 and float(q.max_val) == 5.0
    assert a(b1) is b1 and a(b2) is b2 and a.counter == 0
    assert float(a.max_val) == float(torch.tensor(3.0) + 0.01 * (torch.tensor(5.0) - torch.tensor(3.0)))
    with pytest.raises(RuntimeError, match="ROCm GPU"):   # quantizing has no CPU implementation
        a(b1)
    with pytest.raises(NotImplementedError, match="host loop"):
        aq.get_quant_layer("histogram", "s", bits=8, counter=4)
    with pytest.raises(NotImplementedError):
        aq.get_quant_layer("nope", "s", bits=8)
    # add_quant: a module under its name, a Sequential's children under theirs, the quantizer last
    conv = nn.Conv2d(2, 2, 1)
    w = aq.add_quant("conv1", conv, "minmax", bits=8, counter=4)
    assert [n for n, _ in w.named_children()] == ["conv1", "activation_post_process"] and w.conv1 is conv
    w2 = aq.add_quant("blk", nn.Sequential(nn.Conv2d(2, 2, 1), nn.ReLU()), "fixed", bits=4, zero_point=0.0, scope=1.0)
    assert [n for n, _ in w2.named_children()] == ["0", "1", "activation_post_process"]
    assert w2.activation_post_process.name == "blk_quant"
    # collect: in stage order, None for a stage without a range
    seq = nn.Sequential()
    seq.add_module("conv1", aq.add_quant("conv1", nn.Identity(), "minmax", bits=8, counter=4))
    seq.add_module("conv2", nn.Identity())
    seq.add_module("conv3", aq.add_quant("conv3", nn.Identity(), "avgminmax", bits=4, counter=4))
    seq.conv1(b1)
    assert aq.collect(seq) == [(8, -2.0, 3.0), None, None]
    seq.conv3(b2)
    assert aq.collect(seq) == [(8, -2.0, 3.0), None, (4, 0.0, 5.0)]


def _host_packed(shape, bits=4):
    from admmq import PackedTensor
    from admmq.packed import packed_bytes
    n = shape[0] * shape[1]
    return PackedTensor(codes=torch.zeros(packed_bytes(n, bits), dtype=torch.uint8), shape=tuple(shape), bits=bits,
                        qscheme="tensor_symmetric", scale=0.25, zero_point=0, mn=0.0, rng=0.0, index=-1)


def test_packed_modules_carry_their_quantizers():
    from admmq import export
    from admmq.quantization import act_range
    m = export.PackedConv1x1(_host_packed((6, 10)))
    old_state = {k: v for k, v in m.get_extra_state().items() if k != "act"}   # as written before the quantizers
    assert m.get_extra_state()["act"] is None and "act=" not in m.extra_repr()
    m.set_activation_quant(4, 0.3, 1.4)
    mn, rng = act_range(0.3, 1.4)
    assert m.get_extra_state()["act"] == [4, mn, rng] and f"act=(bits=4, mn={mn}, rng={rng})" in m.extra_repr()
    fresh = export.PackedConv1x1(_host_packed((6, 10)))
    fresh.load_state_dict(m.state_dict())
    assert fresh._act == (4, mn, rng)
    fresh.set_extra_state(old_state)          # a state without the key: no quantizer
    assert fresh._act is None
    m.set_activation_quant(None)
    assert m._act is None
    with pytest.raises(ValueError, match="1..24"):
        m.set_activation_quant(25, 0.0, 1.0)
    d = export.PackedDepthwiseConv1x1(_host_packed((6, 10)), torch.zeros(9, 10), None, (3, 3), 1, 1)
    old_d = {k: v for k, v in d.get_extra_state().items() if k not in ("act", "mid_act")}
    d.set_mid_activation_quant(8, torch.tensor(-1.0), torch.tensor(2.0))
    d.set_activation_quant(4, 0.0, 1.0)
    st = d.get_extra_state()
    assert st["mid_act"] == [8, -1.0, 3.0] and st["act"] == [4, 0.0, 1.0]
    assert "mid_act=(bits=8, mn=-1.0, rng=3.0)" in d.extra_repr() and "act=(bits=4" in d.extra_repr()
    d2 = export.PackedDepthwiseConv1x1(_host_packed((6, 10)), torch.zeros(9, 10), None, (3, 3), 1, 1)
    d2.load_state_dict(d.state_dict())
    assert d2._mid_act == (8, -1.0, 3.0) and d2._act == (4, 0.0, 1.0)
    d2.set_extra_state(old_d)
    assert d2._mid_act is None and d2._act is None
    d.set_mid_activation_quant(None)
    assert d._mid_act is None and d._act is not None


def test_builders_take_act_quant():
    from torch import nn
    from admmq import actquant as aq, export
    A, B, C = _host_packed((8, 5)), _host_packed((6, 5)), _host_packed((9, 5))
    acts = [(8, -1.0, 1.0), (4, 0.3, 1.4), None]
    # (a packed 3-way layer de-quantizes its C factor on the device: tests/test_gpu_actquant.py builds those)
    fl = export.build_cp_layer(5, [torch.zeros(8, 5), torch.zeros(6, 5), torch.zeros(9, 5)], None, 6, 8, (3, 3), 1, 1,
                               act_quant=acts)
    assert [type(getattr(fl, n)) for n in ("conv1", "conv2", "conv3")] == [nn.Sequential, nn.Sequential, nn.Conv2d]
    assert [n for n, _ in fl.conv2.named_children()] == ["conv2", "activation_post_process"]
    assert type(fl.conv2.activation_post_process) is aq.FixedQuant and fl.conv2.activation_post_process.bits == 4
    assert aq.collect(fl) == acts
    two = export.build_cp2conv_layer(5, [A, B], None, 6, 8, 0, 1, act_quant=acts[:2])
    assert two.conv1._act[0] == 8 and two.conv2._act[0] == 4
    fc = export.build_cpfc_layer(5, [A, B], None, 6, 8, act_quant=acts[:2])
    assert fc.fc1._act[0] == 8 and fc.fc2._act[0] == 4
    conv = nn.Conv2d(6, 8, 3, padding=1, bias=False)
    conv1 = nn.Conv2d(6, 8, 1, bias=False)
    assert export.factorized_conv(conv1, 5, [A, B], act_quant=acts[:2]).conv1._act[0] == 8
    for call in (lambda: export.build_cp_layer(5, [A, B, C], None, 6, 8, (3, 3), 1, 1, act_quant=acts[:2]),
                 lambda: export.build_cp2conv_layer(5, [A, B], None, 6, 8, 0, 1, act_quant=acts),
                 lambda: export.build_cpfc_layer(5, [A, B], None, 6, 8, act_quant=acts),
                 lambda: export.factorized_conv(conv, 5, [A, B, C], fused=True, act_quant=acts + [None])):
        with pytest.raises(ValueError, match="act_quant needs"):
            call()
