"""Factorized-layer export: CP / low-rank factors -> drop-in ``nn.Sequential`` layers.

Same names, arguments, module layout (``conv1/conv2/conv3``, ``fc1/fc2``, ``vh/u``)
and weight shapes as ``source/models.py:24-122`` (``build_cp_layer``,
``build_cp2conv_layer``, ``build_cpfc_layer``, ``build_svd_layer``), so a model patched
by ``scripts/calibrate.py:150-187`` can take them unchanged. Factors stay on the
device they were produced on (the reference round-trips them through ``.pt`` files):

* 3-way CP of a ``k x k`` conv weight ``W[o, i, h, w] = sum_r A[o,r] B[i,r] C[h k + w, r]``
  becomes 1x1 (B^T) -> depthwise k x k (C) -> 1x1 (A) + bias.
* 2-way CP of a 1x1 conv / linear ``W = A B^T`` becomes two 1x1 convs / linears.

``load_factors`` reads the files ``admmq.factorize.main`` writes, with the
``scripts/calibrate.py:169-184`` naming (``weights_only=True``); ``packed=True`` reads the
packed integer codes of ``--save-packed`` and de-quantizes them on the device.

Packed layers: ``load_packed_factors`` returns the ``PackedTensor`` factors themselves, and
the CP builders accept them in place of float tensors: the 1x1 convs / linears then become
``PackedConv1x1`` / ``PackedLinear``, which keep the codes and run ``k_packed_gemm`` on them
(inference only); no float32 copy of such a factor is ever made. ``fused=True`` replaces a
3-way layer's ``conv2`` / ``conv3`` by one ``PackedDepthwiseConv1x1`` (``k_packed_dwgemm``).
``integer=True`` (2-way builders) returns an ``IntegerPackedPair``: the input is encoded to
activation codes once and both stages run on ``k_packed_igemm`` (int8 MFMA), codes to codes to float.
``build_qlr_layer`` turns the ``PackedLowRank`` of ``admmq.lowrank`` (``W ~ W_q + L Rt``) into a
``PackedLowRankLinear``: codes and thin factors, one GEMM (``k_packed_lrgemm``).
``integer=True`` of ``build_cp_layer`` returns an ``IntegerPackedCP``: ``conv1`` on ``k_packed_igemm`` and
the fused depthwise + 1x1 stage on ``k_packed_idwgemm`` (an int8 stencil feeding the int8 MFMA).
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _lib
from .packed import (PackedLowRank, PackedTensor, QuantizedActivation, _idwgemm, _int_weight_dims, _lowrank_dims,
                     _meta_words, _pair, _weight_dims, _igemm, act_encode, load_packed, packed_bytes, packed_dwgemm,
                     packed_gemm, packed_lrgemm, packed_rowsums, packed_taps_int, taps_kp)


def _param(t: torch.Tensor) -> nn.Parameter:
    return nn.Parameter(t.detach().clone().contiguous(), requires_grad=True)


def _expect(module_w: torch.Tensor, t: torch.Tensor):
    if tuple(module_w.shape) != tuple(t.shape):
        raise AssertionError(f'Expected shape: {tuple(module_w.shape)}, but got {tuple(t.shape)}')


def _expect_shape(expected, got):
    if tuple(expected) != tuple(got):
        raise AssertionError(f'Expected shape: {tuple(expected)}, but got {tuple(got)}')


def _is_packed(factors) -> bool:
    return bool(factors) and all(isinstance(f, PackedTensor) for f in factors)


class _PackedWeight(nn.Module):
    """A weight ``[out, in]`` kept as the packed codes of ``p`` (``transpose``: ``p`` holds its
    transpose ``[in, out]``). ``codes`` is a uint8 buffer; the scale / zero-point / shape travel
    in the extra state; ``bias`` is an optional parameter (``requires_grad=False``: the layer is
    inference only). There is no ``weight`` attribute: ``dequantize()`` returns the float32
    weight for callers that want the library GEMM instead. A bfloat16 / float16 input runs on the
    16-bit MFMA and gives an output of its dtype; ``module.half()`` leaves the codes
    and the quantization record untouched and turns only the bias into half (it is read as float32,
    exactly). The output quantizer needs float32 activations."""
    _layout = 1

    def __init__(self, p: PackedTensor, bias: Optional[torch.Tensor] = None, transpose: bool = False):
        super().__init__()
        self.transpose = bool(transpose)
        self.out_features, self.in_features = _weight_dims(p, self.transpose)
        self.register_buffer("codes", p.codes.detach().clone().contiguous())
        self._set_quant(p)
        self._act = None   # output quantizer: (bits, mn, rng) as resolved float32 values, or None
        if bias is not None:
            _expect_shape((self.out_features,), bias.shape)
            self.bias = nn.Parameter(bias.detach().clone().to(self.codes.device).contiguous(), requires_grad=False)
        else:
            self.register_parameter("bias", None)

    def _set_quant(self, p):
        self._q = dict(shape=[int(s) for s in p.shape], bits=int(p.bits), qscheme=str(p.qscheme), scale=float(p.scale),
                       zero_point=int(p.zero_point), mn=float(p.mn), rng=float(p.rng), index=int(p.index))
        self._meta = _meta_words(self.packed())

    def packed(self) -> PackedTensor:
        """The layer's weight as a ``PackedTensor`` sharing the ``codes`` buffer."""
        q = self._q
        return PackedTensor(codes=self.codes, shape=tuple(q["shape"]), bits=q["bits"], qscheme=q["qscheme"],
                            scale=q["scale"], zero_point=q["zero_point"], mn=q["mn"], rng=q["rng"], index=q["index"])

    def dequantize(self) -> torch.Tensor:
        """The float32 weight ``[out, in]`` (a new tensor; the layer does not keep it)."""
        w = self.packed().dequantize()
        return w.T.contiguous() if self.transpose else w

    @staticmethod
    def _resolve_act(bits, min_val, max_val):
        if bits is None:
            return None
        from .quantization import act_range, act_record
        mn, rng = act_range(min_val, max_val)
        act_record(bits, mn, rng)   # (refuses bits outside 1..24)
        return (int(bits), mn, rng)

    @staticmethod
    def _act_arg(a):
        return None if a is None else _lib.ActQ(a[0], 1, a[1], a[2])

    def set_activation_quant(self, bits=None, min_val=None, max_val=None):
        """The fixed-range quantizer of the layer's output, applied in the kernel's epilogue
        (``min_max_quantize(y, bits, min_val, max_val)``'s bits); ``None`` clears it."""
        self._act = self._resolve_act(bits, min_val, max_val)

    def get_extra_state(self):
        return dict(self._q, transpose=self.transpose, act=list(self._act) if self._act else None)

    def set_extra_state(self, state):
        q = {k: state[k] for k in ("shape", "bits", "qscheme", "scale", "zero_point", "mn", "rng", "index")}
        if bool(state["transpose"]) != self.transpose or [int(s) for s in q["shape"]] != self._q["shape"] or \
                packed_bytes(self.in_features * self.out_features, int(q["bits"])) != self.codes.numel():
            raise ValueError(f"packed state of shape {tuple(q['shape'])}, {q['bits']} bits, transpose={state['transpose']} "
                             f"does not fit this layer ({tuple(self._q['shape'])}, {self._q['bits']} bits, "
                             f"transpose={self.transpose})")
        self._set_quant(PackedTensor(codes=self.codes, shape=tuple(q["shape"]), bits=int(q["bits"]), qscheme=q["qscheme"],
                                     scale=float(q["scale"]), zero_point=int(q["zero_point"]), mn=float(q["mn"]),
                                     rng=float(q["rng"]), index=int(q["index"])))
        a = state.get("act")   # (absent in states written before the quantizers existed: none)
        self._act = (int(a[0]), float(a[1]), float(a[2])) if a else None

    def _gemm(self, x):
        return packed_gemm(self.codes, self._meta, self.transpose, self.out_features, self.in_features, x, self._layout,
                           self.bias, self._act_arg(self._act))

    def _act_repr(self):
        return "" if self._act is None else f", act=(bits={self._act[0]}, mn={self._act[1]}, rng={self._act[2]})"

    def extra_repr(self):
        return (f"{self.in_features}, {self.out_features}, bits={self._q['bits']}, qscheme={self._q['qscheme']}, "
                f"transpose={self.transpose}, bias={self.bias is not None}{self._act_repr()}")


class PackedLinear(_PackedWeight):
    """``nn.Linear`` on packed codes: ``x [..., in] -> [..., out]``."""
    _layout = 1

    def forward(self, x):
        return self._gemm(x)


class PackedLowRankLinear(_PackedWeight):
    """``nn.Linear`` on the quant + low-rank form ``W = W_q + L Rt`` of ``admmq.lowrank``: ``x [..., in] -> [..., out]``
    by ``k_lr_down`` + ``k_packed_lrgemm``. ``W_q`` stays packed in ``codes``; ``L [out, r]`` and
    ``Rt [r, in]`` are float32 buffers. Neither ``W_q`` nor ``L Rt`` is ever formed. No activation quantizer yet.
    A bfloat16 / float16 input is a composition, not the fused kernel: the half packed GEMM with a float32
    result plus ``(x.float() @ Rt.float().T) @ L.float().T`` and the bias, converted once to the input's dtype."""

    def __init__(self, p: PackedLowRank, bias: Optional[torch.Tensor] = None, act=None):
        if act is not None:
            raise NotImplementedError("PackedLowRankLinear: act= (an output quantizer on the fused quant + low-rank "
                                      "layer) is not supported")
        M, K, r = _lowrank_dims(p)
        super().__init__(p.q, bias, transpose=False)
        dev = self.codes.device
        self.register_buffer("L", p.L.detach().clone().to(dev).contiguous())
        self.register_buffer("Rt", p.Rt.detach().clone().to(dev).contiguous())

    @property
    def rank(self) -> int:
        return int(self.L.shape[1])

    def set_activation_quant(self, bits=None, min_val=None, max_val=None):
        if bits is not None:
            raise NotImplementedError("PackedLowRankLinear: an output quantizer on the fused quant + low-rank layer is "
                                      "not supported")
        self._act = None

    def packed_lowrank(self) -> PackedLowRank:
        """The layer's weight as a ``PackedLowRank`` sharing its buffers."""
        return PackedLowRank(q=self.packed(), L=self.L, Rt=self.Rt)

    def dequantize(self) -> torch.Tensor:
        """``W_q + L Rt`` as a float32 ``[out, in]`` tensor (a new tensor; the layer does not keep it)."""
        return self.packed().dequantize() + self.L @ self.Rt

    def get_extra_state(self):
        return dict(super().get_extra_state(), rank=self.rank)

    def set_extra_state(self, state):
        if int(state.get("rank", -1)) != self.rank:
            raise ValueError(f"packed low-rank state of rank {state.get('rank')} does not fit this layer (rank {self.rank})")
        if state.get("act"):
            raise NotImplementedError("PackedLowRankLinear: a state with an output quantizer is not supported")
        super().set_extra_state(state)

    def forward(self, x):
        return packed_lrgemm(self.codes, self._meta, self.out_features, self.in_features, self.L, self.Rt, x, self.bias)

    def extra_repr(self):
        return (f"{self.in_features}, {self.out_features}, rank={self.rank}, bits={self._q['bits']}, "
                f"qscheme={self._q['qscheme']}, bias={self.bias is not None}")


def build_qlr_layer(p: PackedLowRank, bias: Optional[torch.Tensor] = None) -> PackedLowRankLinear:
    """The linear layer of a quant + low-rank factorization (``factorize_lowrank(..., return_packed=True)`` or
    ``load_packed_lowrank``): ``y = (W_q + L Rt) x + bias`` straight from the codes and the factors."""
    return PackedLowRankLinear(p, bias)


class PackedConv1x1(_PackedWeight):
    """A 1x1 ``nn.Conv2d`` on packed codes: ``x [n, in, H, W] -> [n, out, H', W']``. Zero
    padding and stride act on ``x`` before the product (a 1x1 kernel commutes with both)."""
    _layout = 0

    def __init__(self, p: PackedTensor, bias: Optional[torch.Tensor] = None, transpose: bool = False, stride=1,
                 padding=0):
        super().__init__(p, bias, transpose)
        self.stride = (stride, stride) if isinstance(stride, int) else tuple(stride)
        self.padding = (padding, padding) if isinstance(padding, int) else tuple(padding)

    def forward(self, x):
        if self.padding != (0, 0):
            x = nn.functional.pad(x, (self.padding[1], self.padding[1], self.padding[0], self.padding[0]))
        if self.stride != (1, 1):
            x = x[:, :, ::self.stride[0], ::self.stride[1]]
        return self._gemm(x)


class PackedDepthwiseConv1x1(_PackedWeight):
    """The depthwise ``k x k`` stage and the last 1x1 stage of a 3-way CP layer in one kernel
    (``k_packed_dwgemm``): ``x [n, R, H, W] -> [n, out, Ho, Wo]``. The weight ``A [out, R]`` stays
    packed; ``taps`` is a float32 buffer ``[kh kw, R]`` (the de-quantized ``C`` factor as it is:
    ``k k R`` values). The rank-``R`` tensor between the two stages is never written. Kernel
    size, stride and padding travel in the extra state beside the weight's quantization."""
    _layout = 0

    def __init__(self, p: PackedTensor, taps: torch.Tensor, bias: Optional[torch.Tensor] = None, kernel_size=(3, 3),
                 stride=1, padding=0):
        super().__init__(p, bias, transpose=False)
        self.kernel_size, self.stride, self.padding = _pair(kernel_size, "kernel_size"), _pair(stride, "stride"), \
            _pair(padding, "padding")
        _expect_shape((self.kernel_size[0] * self.kernel_size[1], self.in_features), taps.shape)
        if taps.dtype != torch.float32:
            raise TypeError(f"taps must be float32, got {taps.dtype}")
        self.register_buffer("taps", taps.detach().clone().to(self.codes.device).contiguous())
        self._mid_act = None   # quantizer of the depthwise stage's output (the reference's behind conv2)

    def set_mid_activation_quant(self, bits=None, min_val=None, max_val=None):
        """The fixed-range quantizer of the depthwise stage's output, applied as the kernel stages
        it (the tile's padding stays 0); ``None`` clears it."""
        self._mid_act = self._resolve_act(bits, min_val, max_val)

    def get_extra_state(self):
        return dict(super().get_extra_state(), kernel_size=list(self.kernel_size), stride=list(self.stride),
                    padding=list(self.padding), mid_act=list(self._mid_act) if self._mid_act else None)

    def set_extra_state(self, state):
        if tuple(state["kernel_size"]) != self.kernel_size:
            raise ValueError(f"packed state with kernel size {tuple(state['kernel_size'])} does not fit this layer "
                             f"({self.kernel_size})")
        super().set_extra_state(state)
        self.stride, self.padding = _pair(state["stride"], "stride"), _pair(state["padding"], "padding")
        a = state.get("mid_act")
        self._mid_act = (int(a[0]), float(a[1]), float(a[2])) if a else None

    def forward(self, x):
        return packed_dwgemm(self.codes, self._meta, self.out_features, self.in_features, x, self.taps, self.kernel_size,
                             self.stride, self.padding, self.bias, self._act_arg(self._act), self._act_arg(self._mid_act))

    def extra_repr(self):
        m = "" if self._mid_act is None else \
            f", mid_act=(bits={self._mid_act[0]}, mn={self._mid_act[1]}, rng={self._mid_act[2]})"
        return (f"{super().extra_repr()}, kernel_size={self.kernel_size}, stride={self.stride}, "
                f"padding={self.padding}{m}")


class IntegerPackedPair(nn.Module):
    """A 2-way packed layer that stays in integers from its first stage to its last:
    the float input is encoded once by ``in_act`` (``k_act_encode``), stage 1 runs from codes to
    the codes of its output under the inter-stage quantizer, stage 2 from those codes to a float
    output (quantized where the stage has an output quantizer) - both on ``k_packed_igemm``. The
    children keep the float layer's names and are its ``PackedConv1x1`` / ``PackedLinear`` stages
    (stage 1's output quantizer is the inter-stage one); ``in_act`` and the weights' integer row
    sums travel in this module's extra state. ``last_clamped``: the device counters of the two
    encodings of the last forward (input, inter-stage); no forward reads them."""

    def __init__(self, names, stage1: _PackedWeight, stage2: _PackedWeight, in_act):
        super().__init__()
        self._names = tuple(names)
        self.add_module(names[0], stage1)
        self.add_module(names[1], stage2)
        self._in_act = in_act   # (bits, mn, rng), resolved float32 values
        self._rs = [None, None]
        self.last_clamped = None
        if stage1.codes.device.type == "cuda":
            self._rowsums(0), self._rowsums(1)

    def _stage(self, i):
        return getattr(self, self._names[i])

    def _rowsums(self, i):
        st = self._stage(i)
        if self._rs[i] is None:
            self._rs[i] = packed_rowsums(st.packed(), st.transpose)
        elif self._rs[i].device != st.codes.device:
            self._rs[i] = self._rs[i].to(st.codes.device)
        return self._rs[i]

    def get_extra_state(self):
        return dict(in_act=list(self._in_act), rowsums=[None if r is None else r.detach().cpu() for r in self._rs])

    def set_extra_state(self, state):
        a = state["in_act"]
        self._in_act = (int(a[0]), float(a[1]), float(a[2]))
        rs = []
        for i, r in enumerate(state.get("rowsums") or [None, None]):
            if r is not None and (r.dtype != torch.int32 or tuple(r.shape) != (self._stage(i).out_features,)):
                raise ValueError(f"integer layer state: row sums of stage {i + 1} must be int32 "
                                 f"[{self._stage(i).out_features}], got {r.dtype} {tuple(r.shape)}")
            rs.append(r)
        self._rs = rs

    @torch.compiler.disable
    def forward(self, x):
        s1, s2 = self._stage(0), self._stage(1)
        if isinstance(s1, PackedConv1x1):
            if s1.padding != (0, 0):
                x = nn.functional.pad(x, (s1.padding[1], s1.padding[1], s1.padding[0], s1.padding[0]))
            if s1.stride != (1, 1):
                x = x[:, :, ::s1.stride[0], ::s1.stride[1]]
        xq = act_encode(x, _lib.ActQ(self._in_act[0], 1, self._in_act[1], self._in_act[2]), check=False)
        mid = s1._act
        if mid is None or not 2 <= mid[0] <= 8:
            raise ValueError("integer layer: stage 1 needs its output quantizer with 2 <= bits <= 8 (it writes codes)")
        h = _igemm(s1.codes, s1._meta, s1.transpose, s1.out_features, s1.in_features, xq.codes, self._in_act, self._rowsums(0),
                   s1._layout, s1.bias, mid, True)
        self.last_clamped = (xq.clamped, h.clamped)
        return _igemm(s2.codes, s2._meta, s2.transpose, s2.out_features, s2.in_features, h.codes, mid, self._rowsums(1),
                      s2._layout, s2.bias, s2._act if s2._act is not None else (0, 0.0, 0.0), False)

    def extra_repr(self):
        return f"integer, in_act=(bits={self._in_act[0]}, mn={self._in_act[1]}, rng={self._in_act[2]})"


def _integer_pair(who, names, factors, acts, in_act, make):
    """``integer=True`` of a 2-way builder: argument checks, then the pair over ``make()``'s two stages."""
    if not _is_packed(factors):
        raise ValueError(f"{who}: integer=True needs PackedTensor factors (the integer stages run from packed codes)")
    if in_act is None:
        raise ValueError(f"{who}: integer=True needs in_act, the (bits, min_val, max_val) quantizer of the layer's input")
    if acts[0] is None:
        raise ValueError(f"{who}: integer=True needs the inter-stage entry of act_quant (stage 1 writes codes)")
    for a, what in ((in_act, "in_act"), (acts[0], "the inter-stage quantizer")):
        if not 2 <= int(a[0]) <= 8:
            raise ValueError(f"{who}: {what} needs 2 <= bits <= 8 for activation codes, got {a[0]}")
    stage1, stage2 = make()
    for st in (stage1, stage2):
        _int_weight_dims(st.packed(), st.transpose, who)
    return IntegerPackedPair(names, stage1, stage2, _PackedWeight._resolve_act(*in_act))


def _taps_from_float(taps: torch.Tensor, scale: float) -> torch.Tensor:
    """The int8 tap image of float taps ``[kh kw, K]`` that are ``float(c) * scale`` (a packed factor's
    de-quantization): ``c = round(taps / scale)`` is exact for ``|c| <= 128``. One-off, when a state
    came without the image."""
    img = torch.zeros((taps.shape[0], taps_kp(taps.shape[1])), dtype=torch.int8, device=taps.device)
    if scale != 0.0:   # (a zero scale: every tap is 0 and so is every z, whatever the integers)
        img[:, :taps.shape[1]] = torch.round(taps / scale).to(torch.int8)
    return img


class IntegerPackedCP(nn.Module):
    """A 3-way packed CP layer whose activations are uint8 codes from its input encode to its last
    epilogue: the float input is encoded once by ``in_act`` (``k_act_encode``),
    ``conv1`` (``PackedConv1x1``, ``B^T``) runs from codes to the codes of the rank-``R`` tensor under its
    output quantizer on ``k_packed_igemm``, and ``conv23`` (``PackedDepthwiseConv1x1``) runs the integer
    stencil and the last 1x1 stage on ``k_packed_idwgemm`` under its mid quantizer, to a float output
    (quantized where ``conv23`` has an output quantizer). The children are the ``fused=True`` layout's;
    ``in_act``, the two row-sum vectors, the depthwise factor's scale and its int8 tap image travel in
    this module's extra state. ``last_clamped``: the device counters of the last forward (input encode,
    rank tensor, depthwise output; plus the output's with ``out_codes``); no forward reads them."""

    def __init__(self, conv1: PackedConv1x1, conv23: PackedDepthwiseConv1x1, in_act, taps_scale: float,
                 taps_i8: Optional[torch.Tensor] = None):
        super().__init__()
        self.conv1, self.conv23 = conv1, conv23
        self._in_act = in_act   # (bits, mn, rng), resolved float32 values
        self._taps_scale = float(taps_scale)
        self._taps_i8 = self._check_taps(taps_i8)
        self._rs = [None, None]
        self.out_codes = False   # True (needs conv23's output quantizer, bits 2..8): forward returns codes
        self.last_clamped = None
        if conv1.codes.device.type == "cuda":
            self._rowsums(0), self._rowsums(1), self._taps()

    def _stage(self, i):
        return self.conv1 if i == 0 else self.conv23

    def _rowsums(self, i):
        st = self._stage(i)
        if self._rs[i] is None:
            self._rs[i] = packed_rowsums(st.packed(), st.transpose)
        elif self._rs[i].device != st.codes.device:
            self._rs[i] = self._rs[i].to(st.codes.device)
        return self._rs[i]

    def _check_taps(self, t):
        c = self.conv23
        shape = (c.kernel_size[0] * c.kernel_size[1], taps_kp(c.in_features))
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.int8 or tuple(t.shape) != shape):
            raise ValueError(f"integer layer state: the tap image must be int8 {list(shape)}, got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
        return t

    def _taps(self):
        c = self.conv23
        if self._taps_i8 is None:
            self._taps_i8 = _taps_from_float(c.taps, self._taps_scale)
        elif self._taps_i8.device != c.codes.device:
            self._taps_i8 = self._taps_i8.to(c.codes.device)
        return self._taps_i8

    def get_extra_state(self):
        return dict(in_act=list(self._in_act), rowsums=[None if r is None else r.detach().cpu() for r in self._rs],
                    taps_scale=self._taps_scale, taps_i8=None if self._taps_i8 is None else self._taps_i8.detach().cpu())

    def set_extra_state(self, state):
        a = state["in_act"]
        self._in_act = (int(a[0]), float(a[1]), float(a[2]))
        if "taps_scale" not in state:
            raise ValueError("integer layer state: taps_scale (the depthwise factor's scale) is missing")
        rs = []
        for i, r in enumerate(state.get("rowsums") or [None, None]):
            if r is not None and (r.dtype != torch.int32 or tuple(r.shape) != (self._stage(i).out_features,)):
                raise ValueError(f"integer layer state: row sums of stage {i + 1} must be int32 "
                                 f"[{self._stage(i).out_features}], got {r.dtype} {tuple(r.shape)}")
            rs.append(r)
        taps = self._check_taps(state.get("taps_i8"))
        self._rs, self._taps_i8, self._taps_scale = rs, taps, float(state["taps_scale"])

    @torch.compiler.disable
    def forward(self, x):
        s1, s2 = self.conv1, self.conv23
        a0, mid = s1._act, s2._mid_act
        if a0 is None or not 2 <= a0[0] <= 8:
            raise ValueError("integer layer: conv1 needs its output quantizer with 2 <= bits <= 8 (it writes codes)")
        if mid is None or not 2 <= mid[0] <= 8:
            raise ValueError("integer layer: conv23 needs its mid quantizer with 2 <= bits <= 8 (the depthwise stage "
                             "writes codes)")
        out = s2._act if s2._act is not None else (0, 0.0, 0.0)
        if self.out_codes and not 2 <= out[0] <= 8:
            raise ValueError("integer layer: out_codes needs conv23's output quantizer with 2 <= bits <= 8")
        if s1.padding != (0, 0):
            x = nn.functional.pad(x, (s1.padding[1], s1.padding[1], s1.padding[0], s1.padding[0]))
        if s1.stride != (1, 1):
            x = x[:, :, ::s1.stride[0], ::s1.stride[1]]
        xq = act_encode(x, _lib.ActQ(self._in_act[0], 1, self._in_act[1], self._in_act[2]), check=False)
        h = _igemm(s1.codes, s1._meta, s1.transpose, s1.out_features, s1.in_features, xq.codes, self._in_act, self._rowsums(0),
                   0, s1.bias, a0, True)
        y, midc, outc = _idwgemm(s2.codes, s2._meta, s2.out_features, s2.in_features, h.codes, a0, self._taps(),
                                 self._taps_scale, s2.kernel_size, s2.stride, s2.padding, self._rowsums(1), s2.bias, mid,
                                 out, bool(self.out_codes))
        if self.out_codes:
            self.last_clamped = (xq.clamped, h.clamped, midc, outc)
            return QuantizedActivation(y, out[0], out[1], out[2], outc)
        self.last_clamped = (xq.clamped, h.clamped, midc)
        return y

    def extra_repr(self):
        return f"integer, in_act=(bits={self._in_act[0]}, mn={self._in_act[1]}, rng={self._in_act[2]})"


def _integer_cp(who, rank, factors, bias, cin, cout, kernel_size, padding, stride, groups, acts, in_act):
    """``integer=True`` of the 3-way builder: argument checks, then the integer layer over the fused layout's stages."""
    if not _is_packed(factors):
        raise ValueError(f"{who}: integer=True needs PackedTensor factors (the integer stages run from packed codes)")
    if in_act is None:
        raise ValueError(f"{who}: integer=True needs in_act, the (bits, min_val, max_val) quantizer of the layer's input")
    if acts[0] is None:
        raise ValueError(f"{who}: integer=True needs the conv1 entry of act_quant (conv1 writes codes)")
    if acts[1] is None:
        raise ValueError(f"{who}: integer=True needs the conv2 entry of act_quant (the depthwise stage writes codes)")
    for a, what in ((in_act, "in_act"), (acts[0], "conv1's quantizer"), (acts[1], "conv2's quantizer")):
        if not 2 <= int(a[0]) <= 8:
            raise ValueError(f"{who}: {what} needs 2 <= bits <= 8 for activation codes, got {a[0]}")
    C = factors[2]
    seq = _packed_cp_layer(rank, factors, bias, cin, cout, kernel_size, padding, stride, groups, True, acts)
    for st in (seq.conv1, seq.conv23):
        _int_weight_dims(st.packed(), st.transpose, who)
    _int_weight_dims(C, False, who)
    taps = packed_taps_int(C) if C.codes.device.type == "cuda" else None
    return IntegerPackedCP(seq.conv1, seq.conv23, _PackedWeight._resolve_act(*in_act), float(C.scale), taps)


def _stage_acts(act_quant, n, who):
    """``act_quant`` as a list of ``n`` entries ``(bits, min_val, max_val)`` or ``None`` (``None``: no quantizers)."""
    if act_quant is None:
        return [None] * n
    acts = list(act_quant)
    if len(acts) != n:
        raise ValueError(f"{who}: act_quant needs {n} entries (one per unfused stage, None for none), got {len(acts)}")
    return acts


def _with_act(module, act):
    """A packed stage with its epilogue quantizer set."""
    if act is not None:
        module.set_activation_quant(*act)
    return module


def _wrap_fixed(name, module, act):
    """A float stage followed by a ``FixedQuant`` of the entry's range, laid out as ``add_quant`` does."""
    if act is None:
        return module
    from .actquant import add_quant
    from .quantization import act_range
    mn, rng = act_range(act[1], act[2])
    return add_quant(name, module, 'fixed', bits=int(act[0]), zero_point=mn, scope=rng, min_max=(act[1], act[2]))


def _wrap_all(seq, acts):
    for (name, m), a in zip(list(seq.named_children()), acts):
        setattr(seq, name, _wrap_fixed(name, m, a))
    return seq


def _packed_cp_layer(rank, factors, bias, cin, cout, kernel_size, padding, stride, groups, fused=False, acts=(None,) * 3):
    if groups != 1:
        raise NotImplementedError("packed CP layers support groups=1 only")
    A, B, C = factors
    _expect_shape((rank, cin, 1, 1), (B.shape[1], B.shape[0], 1, 1))
    _expect_shape((kernel_size[0] * kernel_size[1], rank), tuple(C.shape))
    _expect_shape((cout, rank, 1, 1), (A.shape[0], A.shape[1], 1, 1))
    dev = C.codes.device
    if fused:
        conv23 = _with_act(PackedDepthwiseConv1x1(A, C.dequantize(), bias, kernel_size, stride, padding), acts[2])
        if acts[1] is not None:
            conv23.set_mid_activation_quant(*acts[1])
        return nn.Sequential(OrderedDict([
            ('conv1', _with_act(PackedConv1x1(B, None, transpose=True), acts[0])),
            ('conv23', conv23),
        ]))
    conv2 = nn.Conv2d(rank, rank, kernel_size=kernel_size, groups=rank, padding=padding, stride=stride, bias=False,
                      device=dev)
    # k k R floats: nothing to save by keeping the depthwise stage packed; frozen like the
    # packed stages (they refuse an input that requires grad)
    conv2.weight = nn.Parameter(C.dequantize().reshape(*kernel_size, rank).permute(2, 0, 1)[:, None].contiguous(),
                                requires_grad=False)
    return nn.Sequential(OrderedDict([
        ('conv1', _with_act(PackedConv1x1(B, None, transpose=True), acts[0])),
        ('conv2', _wrap_fixed('conv2', conv2, acts[1])),
        ('conv3', _with_act(PackedConv1x1(A, bias, transpose=False), acts[2])),
    ]))


def _packed_cp2conv_layer(rank, factors, bias, cin, cout, padding, stride, acts=(None,) * 2):
    A, B = factors
    _expect_shape((rank, cin, 1, 1), (B.shape[1], B.shape[0], 1, 1))
    _expect_shape((cout, rank, 1, 1), (A.shape[0], A.shape[1], 1, 1))
    return nn.Sequential(OrderedDict([
        ('conv1', _with_act(PackedConv1x1(B, None, transpose=True, stride=stride, padding=padding), acts[0])),
        ('conv2', _with_act(PackedConv1x1(A, bias, transpose=False), acts[1])),
    ]))


def _packed_cpfc_layer(rank, factors, bias, fin, fout, acts=(None,) * 2):
    B, A = factors
    _expect_shape((rank, fin), (A.shape[1], A.shape[0]))
    _expect_shape((fout, rank), tuple(B.shape))
    return nn.Sequential(OrderedDict([
        ('fc1', _with_act(PackedLinear(A, None, transpose=True), acts[0])),
        ('fc2', _with_act(PackedLinear(B, bias, transpose=False), acts[1])),
    ]))


def build_cp_layer(rank: int, factors: Optional[Sequence[torch.Tensor]], bias: Optional[torch.Tensor], cin: int,
                   cout: int, kernel_size: Tuple[int, int], padding, stride, groups: int = 1,
                   fused: bool = False, act_quant=None, integer: bool = False, in_act=None) -> nn.Module:
    """1x1 (cin -> R) -> depthwise kernel_size (R) -> 1x1 (R -> cout); source/models.py:24-51.
    ``PackedTensor`` factors: conv1 / conv3 become ``PackedConv1x1`` (B transposed, A).
    ``fused`` (``PackedTensor`` factors only): the layout is ``conv1`` -> ``conv23``, a
    ``PackedDepthwiseConv1x1`` that runs the depthwise and the last 1x1 stage as one kernel.
    ``act_quant``: ``[conv1, conv2, conv3]`` entries ``(bits, min_val, max_val)`` or ``None`` (as
    ``admmq.actquant.collect`` returns them): packed stages quantize in their epilogue (fused:
    ``conv2``'s entry is ``conv23``'s mid quantizer, ``conv3``'s its output quantizer); a float
    stage is followed by a ``FixedQuant`` the way ``add_quant`` lays it out.
    ``integer`` (``PackedTensor`` factors, ``in_act = (bits, min_val, max_val)`` of the input and the
    ``conv1`` and ``conv2`` entries of ``act_quant``, all with bits 2..8; implies the fused layout): an
    ``IntegerPackedCP`` of ``conv1`` / ``conv23`` whose activations stay uint8 codes between the stages."""
    acts = _stage_acts(act_quant, 3, "build_cp_layer")
    if integer:
        return _integer_cp("build_cp_layer", rank, factors, bias, cin, cout, tuple(kernel_size), padding, stride, groups,
                           acts, in_act)
    if _is_packed(factors):
        return _packed_cp_layer(rank, factors, bias, cin, cout, tuple(kernel_size), padding, stride, groups, fused, acts)
    if fused:
        raise ValueError("build_cp_layer: fused=True needs PackedTensor factors (the fused stage runs from packed codes)")
    dev = factors[0].device if factors else None
    seq = nn.Sequential(OrderedDict([
        ('conv1', nn.Conv2d(cin, rank, kernel_size=(1, 1), groups=groups, bias=False, device=dev)),
        ('conv2', nn.Conv2d(rank, rank, kernel_size=kernel_size, groups=rank, padding=padding, stride=stride,
                            bias=False, device=dev)),
        ('conv3', nn.Conv2d(rank, cout, kernel_size=(1, 1), bias=bias is not None, device=dev)),
    ]))
    if factors:
        A, B, C = factors
        f_cout = A[:, :, None, None]                                        # (cout, R, 1, 1)
        f_cin = B.T[:, :, None, None]                                       # (R, cin, 1, 1)
        f_z = C.reshape(*kernel_size, rank).permute(2, 0, 1)[:, None]       # (R, 1, kh, kw)
        _expect(seq.conv1.weight, f_cin)
        _expect(seq.conv2.weight, f_z)
        _expect(seq.conv3.weight, f_cout)
        with torch.no_grad():
            seq.conv1.weight = _param(f_cin)
            seq.conv2.weight = _param(f_z)
            seq.conv3.weight = _param(f_cout)
            if bias is not None:
                _expect(seq.conv3.bias, bias)
                seq.conv3.bias = _param(bias)
    return _wrap_all(seq, acts)


def build_cp2conv_layer(rank: int, factors: Optional[Sequence[torch.Tensor]], bias: Optional[torch.Tensor], cin: int,
                        cout: int, padding, stride, act_quant=None, integer: bool = False, in_act=None) -> nn.Module:
    """1x1 (cin -> R, with the original padding/stride) -> 1x1 (R -> cout); source/models.py:54-77.
    ``PackedTensor`` factors: both stages become ``PackedConv1x1`` (B transposed, A).
    ``integer`` (``PackedTensor`` factors, ``in_act = (bits, min_val, max_val)`` of the input and the
    ``conv1`` entry of ``act_quant``, both with bits 2..8): an ``IntegerPackedPair`` of the same two stages."""
    acts = _stage_acts(act_quant, 2, "build_cp2conv_layer")   # [conv1, conv2], as build_cp_layer's
    if integer:
        return _integer_pair("build_cp2conv_layer", ("conv1", "conv2"), factors, acts, in_act,
                             lambda: tuple(_packed_cp2conv_layer(rank, factors, bias, cin, cout, padding, stride,
                                                                 acts).children()))
    if _is_packed(factors):
        return _packed_cp2conv_layer(rank, factors, bias, cin, cout, padding, stride, acts)
    dev = factors[0].device if factors else None
    seq = nn.Sequential(OrderedDict([
        ('conv1', nn.Conv2d(cin, rank, kernel_size=(1, 1), padding=padding, stride=stride, bias=False, device=dev)),
        ('conv2', nn.Conv2d(rank, cout, kernel_size=(1, 1), bias=bias is not None, device=dev)),
    ]))
    if factors:
        A, B = factors
        f_cout = A[:, :, None, None]
        f_cin = B.T[:, :, None, None]
        _expect(seq.conv1.weight, f_cin)
        _expect(seq.conv2.weight, f_cout)
        with torch.no_grad():
            seq.conv1.weight = _param(f_cin)
            seq.conv2.weight = _param(f_cout)
            if bias is not None:
                _expect(seq.conv2.bias, bias)
                seq.conv2.bias = _param(bias)
    return _wrap_all(seq, acts)


def build_cpfc_layer(rank: int, factors: Sequence[torch.Tensor], bias: Optional[torch.Tensor], fin: int,
                     fout: int, act_quant=None, integer: bool = False, in_act=None) -> nn.Module:
    """Linear fin -> R (A^T) -> Linear R -> fout (B); source/models.py:80-99 (factors = [B, A]).
    ``PackedTensor`` factors: both stages become ``PackedLinear`` (A transposed, B).
    ``integer``: as ``build_cp2conv_layer``'s, an ``IntegerPackedPair`` of ``fc1`` / ``fc2``."""
    acts = _stage_acts(act_quant, 2, "build_cpfc_layer")   # [fc1, fc2], as build_cp_layer's
    if integer:
        return _integer_pair("build_cpfc_layer", ("fc1", "fc2"), factors, acts, in_act,
                             lambda: tuple(_packed_cpfc_layer(rank, factors, bias, fin, fout, acts).children()))
    if _is_packed(factors):
        return _packed_cpfc_layer(rank, factors, bias, fin, fout, acts)
    B, A = factors
    seq = nn.Sequential(OrderedDict([
        ('fc1', nn.Linear(fin, rank, bias=False, device=A.device)),
        ('fc2', nn.Linear(rank, fout, bias=bias is not None, device=A.device)),
    ]))
    _expect(seq.fc1.weight, A.T)
    _expect(seq.fc2.weight, B)
    with torch.no_grad():
        seq.fc1.weight = _param(A.T)
        seq.fc2.weight = _param(B)
        if bias is not None:
            _expect(seq.fc2.bias, bias)
            seq.fc2.bias = _param(bias)
    return seq


def build_svd_layer(rank: int, U: torch.Tensor, Vh: torch.Tensor, bias: Optional[torch.Tensor], fin: int,
                    fout: int) -> nn.Sequential:
    """Linear fin -> R (Vh) -> Linear R -> fout (U); source/models.py:102-122."""
    seq = nn.Sequential(OrderedDict([
        ('vh', nn.Linear(fin, rank, bias=False, device=U.device)),
        ('u', nn.Linear(rank, fout, bias=bias is not None, device=U.device)),
    ]))
    _expect(seq.u.weight, U)
    _expect(seq.vh.weight, Vh)
    with torch.no_grad():
        seq.u.weight = _param(U)
        seq.vh.weight = _param(Vh)
        if bias is not None:
            _expect(seq.u.bias, bias)
            seq.u.bias = _param(bias)
    return seq


def factor_prefix(outdir_root: str, bits: int, qscheme: str, method: str, seed: int, layer: str, init: str,
                  rank: int) -> str:
    """File prefix of scripts/factorize.py:164-166 / scripts/calibrate.py:169-171."""
    return os.path.join(outdir_root, f"{bits}bit_{qscheme}", f"factors_{method}_seed{seed}",
                        f"{layer}_{method}_{init}_rank_{rank}_")


def load_factors(prefix: str, ndim: int, device=None, packed: bool = False) -> List[torch.Tensor]:
    """``mode_0.pt`` .. ``mode_{ndim-1}.pt`` under ``prefix`` (scripts/calibrate.py:174-181).
    ``packed``: read ``mode_{m}_packed.pt`` (``admmq.factorize --save-packed``) instead and
    return the de-quantized float32 factors on ``device`` (a ROCm GPU; default ``cuda:0``)."""
    if packed:
        from .packed import dequantize_packed, load_packed
        dev = torch.device("cuda:0") if device is None else torch.device(device)
        return dequantize_packed([load_packed(prefix + f"mode_{m}_packed.pt", device=dev) for m in range(ndim)])
    out = []
    for m in range(ndim):
        t = torch.load(prefix + f"mode_{m}.pt", map_location="cpu", weights_only=True)
        if t.dtype != torch.float:
            raise TypeError(f"{prefix}mode_{m}.pt: expected float32 factors, got {t.dtype}")
        out.append(t.to(device) if device is not None else t)
    return out


def load_packed_factors(prefix: str, ndim: int, device=None) -> List[PackedTensor]:
    """The ``PackedTensor`` factors of ``mode_0_packed.pt`` .. ``mode_{ndim-1}_packed.pt`` under
    ``prefix`` (``admmq.factorize --save-packed``), codes on ``device`` (default ``cuda:0``): the
    builders above turn them into packed layers without de-quantizing the large factors."""
    dev = torch.device("cuda:0") if device is None else torch.device(device)
    return [load_packed(prefix + f"mode_{m}_packed.pt", device=dev) for m in range(ndim)]


def factorized_conv(conv: nn.Conv2d, rank: int, factors: Sequence[torch.Tensor], fused: bool = False,
                    act_quant=None, integer: bool = False, in_act=None) -> nn.Module:
    """The replacement scripts/calibrate.py:157-184 builds for ``conv`` from its factors.
    ``fused``: ``build_cp_layer(..., fused=True)`` for a ``k x k`` conv (``PackedTensor`` factors only).
    ``integer`` / ``in_act``: the builders' integer layers (``IntegerPackedCP`` for a ``k x k`` conv,
    ``IntegerPackedPair`` for a 1x1 conv)."""
    bias = conv.bias.detach() if conv.bias is not None else None
    if tuple(conv.kernel_size) != (1, 1):
        return build_cp_layer(rank, list(factors), bias, conv.in_channels, conv.out_channels, conv.kernel_size,
                              conv.padding, conv.stride, conv.groups, fused, act_quant, integer, in_act)
    if fused:
        raise ValueError("factorized_conv: fused=True applies to k x k convs (a 1x1 conv has no depthwise stage)")
    return build_cp2conv_layer(rank, list(factors), bias, conv.in_channels, conv.out_channels, conv.padding,
                               conv.stride, act_quant, integer, in_act)
