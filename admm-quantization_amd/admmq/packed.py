"""Packed integer codes of the tensor quantization schemes (DESIGN.md "Packed codes").

``quantize_packed`` returns, for each tensor, the unsigned ``bits``-wide codes the
quantizer chose - packed into a little-endian bit stream in the tensor's flat row-major
order - together with the scale / zero-point / range that turn them back into exactly
what ``quantize_tensor`` returns (equal under ``torch.equal``; an integer code has no
``-0.0``). The codes come from the kernel that chose the grid (``k_qfinal_pack``), not from
a second guess at the float32 result.

``packed_linear`` / ``packed_conv1x1`` multiply activations by a weight kept as such codes
(``k_packed_gemm``: the codes are decoded inside the GEMM, the float32 weight never exists).
``packed_depthwise_conv1x1`` runs a depthwise ``k x k`` convolution and the 1x1 convolution by
such a weight as one kernel (``k_packed_dwgemm``: the tensor between them is never written).

``act_encode`` turns a float activation into ``QuantizedActivation`` codes (one uint8 per element, the
fixed-range quantizer's level clamped to ``0 .. 2^bits - 1``), and ``packed_linear_int`` /
``packed_conv1x1_int`` multiply such codes by a packed weight in integer arithmetic
(``k_packed_igemm``: int8 MFMA, exact int32 sums, one double-precision epilogue).
``packed_depthwise_conv1x1_int`` is the fused depthwise + 1x1 stage on such codes (``k_packed_idwgemm``: an
int8 stencil over the codes feeds the int8 MFMA).

``PackedLowRank`` is the deployable form of ``admmq.lowrank``'s ``W ~ W_q + W_r``: ``W_q`` as packed
codes, ``W_r`` as its thin factors ``L [M, r]``, ``Rt [r, K]``; ``packed_lowrank_linear`` evaluates
``x (W_q + L Rt)^T (+ bias)`` from the three in one GEMM (``k_lr_down`` + ``k_packed_lrgemm``).

Schemes: ``tensor_mseminmax_symmetric``, ``tensor_minmax`` (``bits >= 2``),
``tensor_symmetric``, ``tensor_affine`` (with its ``tmin`` / ``tmax``); ``bits`` 1..8.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib

__all__ = ["PackedTensor", "quantize_packed", "dequantize_packed", "save_packed", "load_packed", "packed_bytes",
           "packed_gemm", "packed_linear", "packed_conv1x1", "packed_dwgemm", "packed_depthwise_conv1x1",
           "QuantizedActivation", "act_encode", "act_decode", "packed_rowsums", "packed_igemm", "packed_linear_int",
           "packed_conv1x1_int", "packed_taps_int", "packed_depthwise_conv1x1_int", "PackedLowRank",
           "packed_lrgemm", "packed_lowrank_linear", "save_packed_lowrank", "load_packed_lowrank"]

_NAMES = {v: k for k, v in _lib.SCHEMES.items()}
FORMAT = "admmq.packed.v1"
FORMAT_LOWRANK = "admmq.packed_lowrank.v1"
RANK_MAX = 256   # of the fused quant + low-rank GEMM


def packed_bytes(numel: int, bits: int) -> int:
    """Length of the code stream: ``ceil(numel * bits / 8)`` bytes."""
    return (int(numel) * int(bits) + 7) // 8


def _validate(bits: int, qscheme: str) -> int:
    if qscheme in _lib.CHANNEL_SCHEMES:
        raise ValueError(f"{qscheme}: per-channel schemes have no packed form (their output is a broadcast, "
                         "not the tensor's shape)")
    if qscheme not in _lib.SCHEMES:
        raise NotImplementedError(qscheme)
    bits = int(bits)
    if bits < 1 or bits > 8:
        raise ValueError(f"packed codes need 1 <= bits <= 8, got {bits}")
    if qscheme == "tensor_minmax" and bits == 1:
        raise ValueError("tensor_minmax with 1 bit has three output values (sign(x) - 1): no 1-bit code")
    return _lib.SCHEMES[qscheme]


def _meta_words(p: "PackedTensor") -> torch.Tensor:
    """The 8 int32 words of ``admmq_qmeta`` for ``p`` (bad = 0), on the CPU; kept on ``p`` while
    its fields are unchanged (a packed layer asks for them at every forward)."""
    key = (p.qscheme, p.bits, p.scale, p.zero_point, p.mn, p.rng, p.index)
    if getattr(p, "_mw_key", None) == key:
        return p._mw
    f = torch.tensor([p.scale, p.mn, p.rng], dtype=torch.float32).view(torch.int32)
    p._mw = torch.tensor([_lib.SCHEMES[p.qscheme], p.bits, int(f[0]), p.zero_point, int(f[1]), int(f[2]), p.index, 0],
                         dtype=torch.int32)
    p._mw_key = key
    return p._mw


@dataclass
class PackedTensor:
    """One quantized tensor as ``bits``-wide unsigned codes.

    ``codes``: uint8 ``[ceil(numel * bits / 8)]``; element ``i`` of the flat row-major order
    occupies bits ``[i * bits, (i + 1) * bits)`` of the little-endian bit stream.
    ``scale`` / ``zero_point`` (mse-minmax, symmetric, affine) and ``mn`` / ``rng`` (minmax)
    are float32 values held as Python floats (exact); ``index`` is the MSE search's chosen
    candidate, else -1; ``bad`` counts the elements whose result has no valid code (NaN or
    unrepresentable): a tensor with ``bad > 0`` is not a valid packed tensor."""
    codes: torch.Tensor
    shape: Tuple[int, ...]
    bits: int
    qscheme: str
    scale: float
    zero_point: int
    mn: float
    rng: float
    index: int
    bad: int = 0

    @property
    def numel(self) -> int:
        n = 1
        for s in self.shape:
            n *= int(s)
        return n

    @property
    def nbytes(self) -> int:
        return int(self.codes.numel())

    def dequantize(self) -> torch.Tensor:
        """float32 tensor of ``shape`` on the codes' device (``k_dequant_pack``)."""
        return dequantize_packed([self])[0]

    def levels(self) -> torch.Tensor:
        """The unpacked codes, uint8 of ``shape``, on the codes' device (unpacked on the host)."""
        import numpy as np
        b = np.unpackbits(self.codes.detach().cpu().numpy(), bitorder="little")[:self.numel * self.bits]
        w = (1 << np.arange(self.bits, dtype=np.uint16))
        lv = (b.reshape(self.numel, self.bits).astype(np.uint16) * w).sum(axis=1).astype(np.uint8)
        return torch.from_numpy(lv).reshape(self.shape).to(self.codes.device)


def _from_meta(codes, shapes, meta: torch.Tensor, check: bool) -> List[PackedTensor]:
    m = meta.cpu()   # the call's one host sync
    fl = m.view(torch.float32)
    out = []
    for i, (c, shape) in enumerate(zip(codes, shapes)):
        row = m[i].tolist()
        if check and row[7] > 0:
            raise ValueError(f"quantize_packed: tensor {i} has {row[7]} element(s) without a valid code "
                             "(NaN or unrepresentable result; meta.bad > 0)")
        out.append(PackedTensor(codes=c, shape=tuple(shape), bits=row[1], qscheme=_NAMES[row[0]], scale=float(fl[i, 2]),
                                zero_point=row[3], mn=float(fl[i, 4]), rng=float(fl[i, 5]), index=row[6], bad=row[7]))
    return out


def quantize_packed_raw(tensors: Sequence[torch.Tensor], bits: int, qscheme: str, num_attempts: int = 200,
                        tmin: Optional[float] = None, tmax: Optional[float] = None):
    """``(codes, meta)`` on the device without a host sync: uint8 code streams and the int32
    ``[n, 8]`` words of ``admmq_qmeta`` (word 7 = bad)."""
    code = _validate(bits, qscheme)
    xs = []
    for t in tensors:
        _lib.require_device(t)
        if t.numel() == 0:
            raise ValueError("quantize_packed: empty tensor")
        xs.append(t.contiguous())
    if not xs:
        raise ValueError("quantize_packed: no tensors")
    has_kw = code == 3 and tmin is not None and tmax is not None
    if _lib.use_ops():   # torch.ops.admmq.quantize_packed (csrc/torch_ops.cpp) -> admmq_quantize_packed
        codes, meta = _lib.ops().quantize_packed(xs, int(bits), code, int(num_attempts),
                                                 float(tmin) if has_kw else None, float(tmax) if has_kw else None)
        return list(codes), meta
    lib = _lib.load()
    dev = xs[0].device
    items = []
    for x in xs:
        cols = 1 if x.dim() == 0 else x.shape[-1]
        items.append(_lib.QTensor(x.data_ptr(), 0, x.numel() // cols, cols, float(tmin) if has_kw else 0.0,
                                  float(tmax) if has_kw else 0.0, 1 if has_kw else 0, 0))
    arr = _lib.qtensor_array(items)
    codes = [torch.empty(packed_bytes(x.numel(), bits), dtype=torch.uint8, device=dev) for x in xs]
    cptr = (ctypes.c_void_p * len(xs))(*[c.data_ptr() for c in codes])
    meta = torch.empty((len(xs), 8), dtype=torch.int32, device=dev)
    nb = lib.admmq_quantize_packed_workspace_size(arr, len(items), int(num_attempts))
    if nb == 0:
        _lib.check(-1, "quantize workspace planning")
    ws = _lib.workspace(nb, dev)
    rc = lib.admmq_quantize_packed(arr, cptr, _lib.ptr(meta), len(items), int(bits), code, int(num_attempts),
                                   _lib.ptr(ws), nb, _lib.stream_handle(dev))
    _lib.check(rc, "quantize_packed")
    return codes, meta


def quantize_packed(tensors: Sequence[torch.Tensor], bits: int, qscheme: str, num_attempts: int = 200,
                    tmin: Optional[float] = None, tmax: Optional[float] = None,
                    check: bool = True) -> List[PackedTensor]:
    """Packed form of ``quantize_tensor(t, bits, qscheme, ...)`` for every ``t`` in ``tensors``:
    one launch sequence, one host sync (the meta records). ``check``: raise ``ValueError``
    naming the first tensor whose result has no valid code (``bad > 0``: NaN outputs, e.g. an
    all-zero tensor under mse-minmax); with ``check=False`` the count is in ``.bad``."""
    tensors = list(tensors)
    codes, meta = quantize_packed_raw(tensors, bits, qscheme, num_attempts, tmin, tmax)
    return _from_meta(codes, [t.shape for t in tensors], meta, check)


def dequantize_packed(packed: Sequence[PackedTensor]) -> List[torch.Tensor]:
    """float32 tensors of the packed tensors' shapes, one launch for the whole list."""
    packed = list(packed)
    if not packed:
        return []
    dev = packed[0].codes.device
    if dev.type != "cuda":
        raise RuntimeError("admmq: packed codes must live on a ROCm GPU to be de-quantized (device 'cuda'); "
                           "load_packed(path, device=...) puts them there")
    codes, numel = [], []
    for p in packed:
        _validate(p.bits, p.qscheme)
        if p.codes.dtype != torch.uint8 or p.codes.numel() != packed_bytes(p.numel, p.bits) or p.numel == 0:
            raise ValueError(f"packed tensor of shape {tuple(p.shape)} with {p.bits} bits needs "
                             f"{packed_bytes(p.numel, p.bits)} uint8 code bytes")
        if p.codes.device != dev:
            raise RuntimeError("admmq: the packed tensors of one call must share a device")
        codes.append(p.codes.contiguous())
        numel.append(p.numel)
    meta = torch.stack([_meta_words(p) for p in packed]).to(dev)
    if _lib.use_ops():
        ys = _lib.ops().dequantize_packed(codes, meta, numel)
    else:
        lib = _lib.load()
        ys = [torch.empty(n, dtype=torch.float32, device=dev) for n in numel]
        cptr = (ctypes.c_void_p * len(codes))(*[c.data_ptr() for c in codes])
        yptr = (ctypes.c_void_p * len(ys))(*[y.data_ptr() for y in ys])
        ne = (ctypes.c_int64 * len(numel))(*numel)
        rc = lib.admmq_dequantize_packed(cptr, _lib.ptr(meta), yptr, ne, len(codes), _lib.stream_handle(dev))
        _lib.check(rc, "dequantize_packed")
    return [y.view(p.shape) for y, p in zip(ys, packed)]


HALF_DTYPES = {torch.float16: 1, torch.bfloat16: 2}   # ADMMQ_DT_F16 / ADMMQ_DT_BF16 (include/admmq.h)


# --- the call frame of the packed GEMM wrappers ---------------------------------
# Plain functions on tensor metadata, shared by the ctypes route of the six wrappers below. None of
# them looks at the device, and each raises what the wrapper it was cut from raised, in that
# wrapper's order.
def _require_gpu(who: str, names: str, x, *others) -> None:
    """The device refusal of wrapper ``who``: ``x`` (which need not be a tensor) and ``others`` on the GPU."""
    ok = isinstance(x, torch.Tensor) and x.device.type == "cuda"
    for t in others:
        ok = ok and t.device.type == "cuda"
    if not ok:
        raise RuntimeError(f"admmq: {who} needs its {names} on a ROCm GPU (device 'cuda'); "
                           "the MI355X path has no CPU implementation")


def _inference_only(who: str, t: torch.Tensor, name: str) -> None:
    """The refusal of a ``t`` (called ``name``) that requires grad while grad mode is on."""
    if t.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"admmq: {who} is inference only (no backward through packed weights): call it "
                           f"under torch.no_grad() or detach {name}")


def _gemm_geometry(who: str, x: torch.Tensor, M: int, K: int, x_layout: int):
    """``(oshape, nb, N, xc)`` of a GEMM on ``x``: layout 0 ``[nb, K, ...] -> [nb, M, ...]``, layout 1
    ``[..., K] -> [..., M]`` (``nb`` 1); ``N`` columns per batch entry, ``xc`` the contiguous ``x``."""
    if x_layout == 0:
        if x.dim() < 3 or x.shape[1] != K:
            raise ValueError(f"{who}: x must be [n, {K}, ...], got {tuple(x.shape)}")
        oshape = (x.shape[0], M) + tuple(x.shape[2:])
        nb = int(x.shape[0])
    elif x_layout == 1:
        if x.dim() < 1 or x.shape[-1] != K:
            raise ValueError(f"{who}: x must be [..., {K}], got {tuple(x.shape)}")
        oshape = tuple(x.shape[:-1]) + (M,)
        nb = 1
    else:
        raise ValueError(f"{who}: x_layout must be 0 or 1")
    xc = x.contiguous()
    if xc.numel() == 0:
        raise ValueError(f"{who}: empty x")
    return oshape, nb, xc.numel() // (nb * K), xc


def _dw_x_shape(who: str, x: torch.Tensor, K: int) -> None:
    """The shape refusal of a fused depthwise + 1x1 call's ``x``. Apart from ``_dw_geometry``: both
    depthwise wrappers check their tap tensor between this and the empty-x refusal."""
    if x.dim() != 4 or x.shape[1] != K:
        raise ValueError(f"{who}: x must be [n, {K}, H, W], got {tuple(x.shape)}")


def _dw_geometry(who: str, x: torch.Tensor, ks, st, pd):
    """``(nb, H, W, Ho, Wo, xc)`` of a fused depthwise + 1x1 call on a checked ``x [nb, K, H, W]``. A
    geometry outside the limits leaves ``Ho`` / ``Wo`` meaningless: the C call refuses it before any launch."""
    xc = x.contiguous()
    if xc.numel() == 0:
        raise ValueError(f"{who}: empty x")
    nb, H, W = int(xc.shape[0]), int(xc.shape[2]), int(xc.shape[3])
    Ho = max((H + 2 * pd[0] - ks[0]) // max(st[0], 1) + 1, 1)
    Wo = max((W + 2 * pd[1] - ks[1]) // max(st[1], 1) + 1, 1)
    return nb, H, W, Ho, Wo, xc


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """``t`` contiguous at a 16-byte aligned address (a view into a larger buffer is cloned)."""
    tc = t.contiguous()
    return tc.clone() if tc.data_ptr() % 16 else tc


def _weight_arg(codes: torch.Tensor, meta_words: torch.Tensor):
    """The aligned code stream and the C meta record of a packed weight."""
    return _aligned(codes), _lib.QMeta.from_buffer_copy(meta_words.contiguous().numpy().tobytes())


def _bias_arg(who: str, bias: Optional[torch.Tensor], M: int) -> Optional[torch.Tensor]:
    """``None`` or the contiguous float32 ``bias [M]`` on the GPU."""
    if bias is None:
        return None
    _lib.require_device(bias)
    if tuple(bias.shape) != (M,):
        raise ValueError(f"{who}: bias must be [{M}], got {tuple(bias.shape)}")
    return bias.contiguous()


def _actq(t3) -> Optional["_lib.ActQ"]:
    """The C record of a checked quantizer ``(bits, mn, rng)``; bits 0 (none): ``None``."""
    return _lib.ActQ(t3[0], 1, t3[1], t3[2]) if t3[0] else None


def _byref(rec):
    return ctypes.byref(rec) if rec is not None else None


def packed_gemm(codes: torch.Tensor, meta_words: torch.Tensor, transpose: bool, M: int, K: int, x: torch.Tensor,
                x_layout: int, bias: Optional[torch.Tensor] = None, act=None, out_dtype=None) -> torch.Tensor:
    """``Y = W X (+ bias)`` with ``W`` the ``[M, K]`` de-quantization of ``codes`` (``transpose``: of the
    ``[K, M]`` packed tensor's transpose). ``meta_words``: the 8 int32 words of the meta record on
    the CPU. ``x_layout`` 0: ``x [n, K, ...] -> [n, M, ...]``; 1: ``x [..., K] -> [..., M]``.
    ``act = (bits, min_val, max_val)``: the fixed-range activation quantizer of ``min_max_quantize``
    applied to the output inside the kernel (``admmq_packed_gemm_act``): the bits of quantizing the
    result in a launch of its own. A ``torch.bfloat16`` / ``torch.float16`` ``x`` runs on the 16-bit MFMA
    (``admmq_packed_hgemm``): the result has ``x``'s dtype, or float32 with
    ``out_dtype=torch.float32``; ``bias`` may be float32 or of ``x``'s dtype; ``act`` is not available
    there. Inference only: an ``x`` that requires grad is refused while grad mode is on."""
    _require_gpu("packed_gemm", "codes and activations", x, codes)
    if x.dtype in HALF_DTYPES:
        return _packed_hgemm(codes, meta_words, transpose, M, K, x, x_layout, bias, act, out_dtype)
    _lib.require_device(x)
    if out_dtype is not None and out_dtype != torch.float32:
        raise ValueError(f"packed_gemm: a float32 x gives a float32 result, not out_dtype={out_dtype}")
    _inference_only("packed_gemm", x, "x")
    if torch.compiler.is_compiling():   # (see _opaque_packed_gemm below)
        return _opaque_packed_gemm(codes, meta_words, transpose, M, K, x, x_layout, bias, act)
    M, K, x_layout = int(M), int(K), int(x_layout)
    if bias is not None:
        bias = bias.detach()
    oq = _act_record(act)
    if oq is not None and _lib.use_ops():   # torch.ops.admmq.packed_gemm_act -> admmq_packed_gemm_act
        return _lib.ops().packed_gemm_act(codes, meta_words, bool(transpose), M, K, x, x_layout, bias, oq.bits, oq.mn, oq.rng)
    if _lib.use_ops():   # torch.ops.admmq.packed_gemm (csrc/torch_ops.cpp) -> admmq_packed_gemm
        return _lib.ops().packed_gemm(codes, meta_words, bool(transpose), M, K, x, x_layout, bias)
    lib = _lib.load()
    oshape, nb, N, xc = _gemm_geometry("packed_gemm", x, M, K, x_layout)
    (cc, meta), bc = _weight_arg(codes, meta_words), _bias_arg("packed_gemm", bias, M)
    y = torch.empty(oshape, dtype=torch.float32, device=x.device)
    ws = _lib.workspace(lib.admmq_packed_gemm_workspace_size(M, K, N, nb), x.device)
    if oq is not None:
        rc = lib.admmq_packed_gemm_act(_lib.ptr(cc), ctypes.byref(meta), 1 if transpose else 0, M, K, _lib.ptr(xc),
                                       x_layout, N, nb, _lib.ptr(bc), _lib.ptr(y), ctypes.byref(oq), _lib.ptr(ws),
                                       ws.numel(), _lib.stream_handle(x.device))
        _lib.check(rc, "packed_gemm_act")
        return y
    rc = lib.admmq_packed_gemm(_lib.ptr(cc), ctypes.byref(meta), 1 if transpose else 0, M, K, _lib.ptr(xc), x_layout, N,
                               nb, _lib.ptr(bc), _lib.ptr(y), _lib.ptr(ws), ws.numel(), _lib.stream_handle(x.device))
    _lib.check(rc, "packed_gemm")
    return y


def _act_record(act):
    """``None`` or the C record of ``act = (bits, min_val, max_val)`` (the range by ``act_range``); a
    record is taken as it is."""
    if act is None or isinstance(act, _lib.ActQ):
        return act
    from .quantization import act_range, act_record
    bits, lo, hi = act
    return act_record(bits, *act_range(lo, hi))


# Under torch.compile a packed call stays opaque: the meta record is a host tensor (the host picks
# the kernel from its bits) beside GPU tensors, a mix the tracer's fake-tensor device propagation
# refuses. The call is a graph break and runs as it does in eager mode; eager calls do not pass here.
_opaque_packed_gemm = torch.compiler.disable(packed_gemm)


def _packed_hgemm(codes, meta_words, transpose, M, K, x, x_layout, bias, act, out_dtype):
    """``packed_gemm`` on a bfloat16 / float16 ``x`` already known to be on the GPU (``admmq_packed_hgemm``)."""
    if act is not None:
        raise ValueError(f"packed_gemm: act= (an output quantizer) is not available for a {x.dtype} x; it needs "
                         "float32 activations")
    if out_dtype is not None and out_dtype != torch.float32 and out_dtype != x.dtype:
        raise ValueError(f"packed_gemm: out_dtype must be None, torch.float32 or x's dtype {x.dtype}, got {out_dtype}")
    _inference_only("packed_gemm", x, "x")
    if torch.compiler.is_compiling():   # opaque under torch.compile, like the float32 call
        return _opaque_packed_hgemm(codes, meta_words, transpose, M, K, x, x_layout, bias, act, out_dtype)
    M, K, x_layout = int(M), int(K), int(x_layout)
    out_f32 = out_dtype == torch.float32
    if bias is not None:
        if not isinstance(bias, torch.Tensor):
            raise TypeError(f"admmq: expected a torch.Tensor, got {type(bias).__name__}")
        if bias.device.type != "cuda":
            raise RuntimeError("admmq: tensors must live on a ROCm GPU (device 'cuda'); the MI355X path has "
                               "no CPU implementation")
        if bias.dtype != torch.float32 and bias.dtype != x.dtype:
            raise TypeError(f"admmq: packed_gemm: bias must be float32 or x's dtype {x.dtype}, got {bias.dtype}")
        bias = bias.detach().float()   # (exact)
    if _lib.use_ops():   # torch.ops.admmq.packed_hgemm (csrc/torch_ops.cpp) -> admmq_packed_hgemm
        return _lib.ops().packed_hgemm(codes, meta_words, bool(transpose), M, K, x, x_layout, bias, out_f32)
    lib = _lib.load()
    oshape, nb, N, xc = _gemm_geometry("packed_gemm", x, M, K, x_layout)
    (cc, meta), bc = _weight_arg(codes, meta_words), _bias_arg("packed_gemm", bias, M)
    xdt = HALF_DTYPES[x.dtype]
    y = torch.empty(oshape, dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    ws = _lib.workspace(lib.admmq_packed_hgemm_workspace_size(ctypes.byref(meta), M, K, N, nb), x.device)
    rc = lib.admmq_packed_hgemm(_lib.ptr(cc), ctypes.byref(meta), 1 if transpose else 0, M, K, _lib.ptr(xc), xdt,
                                x_layout, N, nb, _lib.ptr(bc), _lib.ptr(y), 0 if out_f32 else xdt, _lib.ptr(ws),
                                ws.numel(), _lib.stream_handle(x.device))
    _lib.check(rc, "packed_hgemm")
    return y


_opaque_packed_hgemm = torch.compiler.disable(_packed_hgemm)


def _weight_dims(p: "PackedTensor", transpose: bool) -> Tuple[int, int]:
    _validate(p.bits, p.qscheme)
    if len(p.shape) != 2:
        raise ValueError(f"a packed weight must be 2-D, got shape {tuple(p.shape)}")
    if p.bad:
        raise ValueError(f"packed tensor has {p.bad} element(s) without a valid code (bad > 0)")
    if p.codes.dtype != torch.uint8 or p.codes.numel() != packed_bytes(p.numel, p.bits) or p.numel == 0:
        raise ValueError(f"packed tensor of shape {tuple(p.shape)} with {p.bits} bits needs "
                         f"{packed_bytes(p.numel, p.bits)} uint8 code bytes")
    r, c = int(p.shape[0]), int(p.shape[1])
    return (c, r) if transpose else (r, c)


def packed_linear(x: torch.Tensor, p: "PackedTensor", bias: Optional[torch.Tensor] = None,
                  transpose: bool = False, act=None, out_dtype=None) -> torch.Tensor:
    """``F.linear(x, W, bias)`` with ``W = p.dequantize()`` (``transpose``: its transpose) computed
    from the codes: ``x [..., K] -> [..., M]``. A bfloat16 / float16 ``x`` gives a result of its dtype
    (float32 with ``out_dtype=torch.float32``), as ``packed_gemm``. Inference only."""
    M, K = _weight_dims(p, transpose)
    return packed_gemm(p.codes, _meta_words(p), transpose, M, K, x, 1, bias, act, out_dtype)


def packed_conv1x1(x: torch.Tensor, p: "PackedTensor", bias: Optional[torch.Tensor] = None, transpose: bool = False,
                   stride=1, act=None, out_dtype=None) -> torch.Tensor:
    """``F.conv2d(x, W[:, :, None, None], bias, stride=stride)`` with ``W = p.dequantize()``
    (``transpose``: its transpose) computed from the codes: ``x [n, K, H, W] -> [n, M, H', W']``.
    The stride sub-samples ``x`` (a 1x1 kernel without padding commutes with it). A bfloat16 / float16 ``x``
    gives a result of its dtype (float32 with ``out_dtype=torch.float32``), as ``packed_gemm``. Inference only."""
    M, K = _weight_dims(p, transpose)
    if isinstance(x, torch.Tensor) and x.dim() != 4:
        raise ValueError(f"packed_conv1x1: x must be [n, {K}, H, W], got {tuple(x.shape)}")
    sh, sw = (stride, stride) if isinstance(stride, int) else tuple(stride)
    if (sh, sw) != (1, 1) and isinstance(x, torch.Tensor):
        x = x[:, :, ::sh, ::sw]
    return packed_gemm(p.codes, _meta_words(p), transpose, M, K, x, 0, bias, act, out_dtype)


# --- integer route -------------------------------------------------------------
INT_K_MAX = 65536   # 128 * 255 * K must stay below 2^31


def _code_act(act, who: str) -> "_lib.ActQ":
    """The C record of a code quantizer ``act = (bits, min_val, max_val)`` (or a record): bits 2..8."""
    if act is None:
        raise ValueError(f"{who}: an activation quantizer (bits, min_val, max_val) is needed")
    q = _act_record(act)
    if not 2 <= int(q.bits) <= 8:
        raise ValueError(f"{who}: activation codes need 2 <= bits <= 8, got {q.bits} (1 bit has three output "
                         "values and no code form)")
    return q


@dataclass
class QuantizedActivation:
    """An activation as codes: ``codes`` uint8 of the float tensor's shape, ``x = (u * rng) / n + mn``
    with ``n = 2^bits - 1`` (``mn`` / ``rng`` float32 values held as Python floats). ``clamped``: an
    int32 ``[1]`` tensor on the codes' device, the number of elements whose level lay outside
    ``0 .. n`` (or was NaN) and was clamped when the codes were made."""
    codes: torch.Tensor
    bits: int
    mn: float
    rng: float
    clamped: Optional[torch.Tensor] = None

    def dequantize(self) -> torch.Tensor:
        """float32 tensor of the codes' shape (``k_act_decode``): where nothing was clamped, the
        bits of ``fixed_quantize`` on the encoded tensor."""
        return act_decode(self.codes, self.bits, self.mn, self.rng)


def act_encode(x: torch.Tensor, act, check: bool = True) -> QuantizedActivation:
    """The codes of ``x`` under ``act = (bits, min_val, max_val)`` (bits 2..8; the range by
    ``act_range``): the level ``fixed_quantize`` computes, clamped to ``0 .. 2^bits - 1``.
    ``check``: one host read, and a ``ValueError`` when any element was clamped (the clamp is the
    one difference from the clamp-free quantizer); ``check=False`` makes no sync and leaves the
    count in ``.clamped`` on the device. Inference only."""
    q = _code_act(act, "act_encode")
    if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("admmq: act_encode is inference only (no backward through the quantizer): call it under "
                           "torch.no_grad() or detach x")
    _lib.require_device(x)
    if torch.compiler.is_compiling():
        return _opaque_act_encode(x, q, check)
    xc = x.detach().contiguous()
    if _lib.use_ops():   # torch.ops.admmq.act_encode (csrc/torch_ops.cpp) -> admmq_act_encode
        codes, clamped = _lib.ops().act_encode(xc, q.bits, q.mn, q.rng)
    else:
        codes = torch.empty(xc.shape, dtype=torch.uint8, device=xc.device)
        clamped = torch.zeros(1, dtype=torch.int32, device=xc.device)
        if xc.numel():
            _lib.check(_lib.load().admmq_act_encode(_lib.ptr(xc), _lib.ptr(codes), xc.numel(), ctypes.byref(q),
                                                    _lib.ptr(clamped), _lib.stream_handle(xc.device)), "act_encode")
    if check:
        n = int(clamped.item())
        if n:
            raise ValueError(f"act_encode: {n} element(s) lie outside the quantizer's range [mn, mn + rng] (or are NaN) "
                             "and were clamped; pass check=False to accept the clamp")
    return QuantizedActivation(codes, int(q.bits), float(q.mn), float(q.rng), clamped)


_opaque_act_encode = torch.compiler.disable(act_encode)


def act_decode(codes: torch.Tensor, bits: int, mn: float, rng: float) -> torch.Tensor:
    """``(float(u) * rng) / n + mn`` in float32 for every code (``k_act_decode``)."""
    q = _code_act(_lib.ActQ(int(bits), 1, float(mn), float(rng)), "act_decode")
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.uint8:
        raise TypeError("act_decode: codes must be a uint8 tensor")
    if codes.device.type != "cuda":
        raise RuntimeError("admmq: activation codes must live on a ROCm GPU (device 'cuda'); the MI355X path has no "
                           "CPU implementation")
    cc = codes.contiguous()
    if _lib.use_ops():
        return _lib.ops().act_decode(cc, q.bits, q.mn, q.rng)
    y = torch.empty(cc.shape, dtype=torch.float32, device=cc.device)
    if cc.numel():
        _lib.check(_lib.load().admmq_act_decode(_lib.ptr(cc), _lib.ptr(y), cc.numel(), ctypes.byref(q),
                                                _lib.stream_handle(cc.device)), "act_decode")
    return y


def _int_weight_dims(p: "PackedTensor", transpose: bool, who: str) -> Tuple[int, int]:
    """``_weight_dims`` plus the integer route's refusals (all on the host)."""
    M, K = _weight_dims(p, transpose)
    if p.qscheme == "tensor_minmax":
        raise ValueError(f"{who}: tensor_minmax weights have no integer form (their de-quantization is not "
                         "scale * integer)")
    q = 1 << (int(p.bits) - 1)
    zp = int(p.zero_point) if p.qscheme == "tensor_affine" else 0
    if -q - zp < -128 or q - 1 - zp > 127:
        raise ValueError(f"{who}: zero_point {zp} puts (u - {q}) - zero_point outside int8")
    if K > INT_K_MAX:
        raise ValueError(f"{who}: K = {K} is past the integer route's limit of {INT_K_MAX}")
    return M, K


def _int_plan(p: "PackedTensor", transpose: bool, who: str) -> list:
    """``[M, K, row sums or None]`` of ``p`` in one orientation, kept on ``p`` while its codes and the
    fields they depend on are unchanged (the way the meta words are): the host refusals run once."""
    codes = p.codes
    c = getattr(p, "_ip", None)
    if c is None or c[2] is not codes or c[3] != codes._version or \
            c[0] != (p.qscheme, p.bits, p.zero_point, p.shape, p.bad):
        c = p._ip = ((p.qscheme, p.bits, p.zero_point, p.shape, p.bad), {}, codes, codes._version)
    e = c[1].get(transpose)
    if e is None:
        e = c[1][transpose] = [*_int_weight_dims(p, transpose, who), None]
    return e


def packed_rowsums(p: "PackedTensor", transpose: bool = False) -> torch.Tensor:
    """``A[m] = sum_k a[m, k]`` (int32 ``[M]``) of the integer weight ``a = (u - q) - zero_point`` of
    ``p`` (``transpose``: of its transpose), by ``k_packed_rowsum``; kept on ``p`` while its codes
    and fields are unchanged, the way the meta words are."""
    e = _int_plan(p, bool(transpose), "packed_rowsums")
    if e[2] is None:
        if p.codes.device.type != "cuda":
            raise RuntimeError("admmq: packed codes must live on a ROCm GPU (device 'cuda'); the MI355X path has no "
                               "CPU implementation")
        e[2] = _rowsums(p.codes, _meta_words(p), bool(transpose), e[0], e[1])
    return e[2]


@torch.compiler.disable
def _rowsums(codes, meta_words, transpose, M, K):
    if _lib.use_ops():
        return _lib.ops().packed_rowsums(codes, meta_words, transpose, M, K)
    cc, meta = _weight_arg(codes, meta_words)
    A = torch.empty(M, dtype=torch.int32, device=cc.device)
    _lib.check(_lib.load().admmq_packed_rowsums(_lib.ptr(cc), ctypes.byref(meta), 1 if transpose else 0, M, K, _lib.ptr(A),
                                                _lib.stream_handle(cc.device)), "packed_rowsums")
    return A


def _in_triple(xq, who: str) -> Tuple[int, float, float]:
    """``(bits, mn, rng)`` of the input codes' quantizer, checked."""
    if not isinstance(xq, QuantizedActivation):
        raise TypeError(f"{who}: xq must be a QuantizedActivation (act_encode makes one)")
    bits = int(xq.bits)
    if not 2 <= bits <= 8:
        raise ValueError(f"{who}: activation codes need 2 <= bits <= 8, got {bits} (1 bit has three output values "
                         "and no code form)")
    return bits, float(xq.mn), float(xq.rng)


def _out_triple(act, out_codes: bool, who: str) -> Tuple[int, float, float]:
    """``(bits, mn, rng)`` of the output quantizer (bits 0: none), checked; ``act`` as ``packed_gemm``'s."""
    if act is None:
        if out_codes:
            raise ValueError(f"{who}: out_codes=True needs act (the output's quantizer)")
        return 0, 0.0, 0.0
    q = _act_record(act)
    if out_codes and not 2 <= int(q.bits) <= 8:
        raise ValueError(f"{who}: activation codes need 2 <= bits <= 8, got {q.bits} (1 bit has three output values "
                         "and no code form)")
    return int(q.bits), float(q.mn), float(q.rng)


def packed_igemm(codes: torch.Tensor, meta_words: torch.Tensor, transpose: bool, M: int, K: int,
                 xq: QuantizedActivation, rowsums: torch.Tensor, x_layout: int, bias: Optional[torch.Tensor] = None,
                 act=None, out_codes: bool = False):
    """``packed_gemm`` on activation codes in integer arithmetic (``admmq_packed_igemm``): ``xq`` holds
    the uint8 codes of ``x`` and their quantizer, ``rowsums`` is ``packed_rowsums`` of the same weight
    and orientation. The result is a float tensor (quantized by ``act`` when given) or, with
    ``out_codes=True`` (needs ``act``, bits 2..8), a ``QuantizedActivation`` whose codes were formed
    in the kernel's epilogue and whose ``clamped`` count stays on the device. Inference only."""
    x3 = _in_triple(xq, "packed_igemm")
    o3 = _out_triple(act, out_codes, "packed_igemm")
    return _igemm(codes, meta_words, bool(transpose), int(M), int(K), xq.codes, x3, rowsums, int(x_layout), bias, o3,
                  bool(out_codes))


def _igemm(codes, meta_words, transpose, M, K, x, x3, rowsums, x_layout, bias, o3, out_codes):
    """The call behind ``packed_igemm`` on checked quantizers ``x3`` / ``o3 = (bits, mn, rng)``."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
        raise TypeError("packed_igemm: xq.codes must be a uint8 tensor")
    _require_gpu("packed_igemm", "codes and activations", x, codes)
    if torch.compiler.is_compiling():   # opaque under torch.compile, like packed_gemm
        return _opaque_igemm(codes, meta_words, transpose, M, K, x, x3, rowsums, x_layout, bias, o3, out_codes)
    if bias is not None:
        bias = bias.detach()
    if _lib.use_ops():   # torch.ops.admmq.packed_igemm (csrc/torch_ops.cpp) -> admmq_packed_igemm
        y, clamped = _lib.ops().packed_igemm(codes, meta_words, transpose, M, K, x, x3[0], x3[1], x3[2], rowsums,
                                             x_layout, bias, o3[0], o3[1], o3[2], out_codes)
    else:
        lib = _lib.load()
        oshape, nb, N, xc = _gemm_geometry("packed_igemm", x, M, K, x_layout)
        (cc, meta), bc = _weight_arg(codes, meta_words), _bias_arg("packed_igemm", bias, M)
        if rowsums.dtype != torch.int32 or tuple(rowsums.shape) != (M,):
            raise ValueError(f"packed_igemm: rowsums must be int32 [{M}]")
        xr, oq = _actq(x3), _actq(o3)
        y = torch.empty(oshape, dtype=torch.uint8 if out_codes else torch.float32, device=x.device)
        clamped = torch.empty(1 if out_codes else 0, dtype=torch.int32, device=x.device)
        ws = _lib.workspace(lib.admmq_packed_igemm_workspace_size(M, K, N, nb), x.device)
        rc = lib.admmq_packed_igemm(_lib.ptr(cc), ctypes.byref(meta), 1 if transpose else 0, M, K, _lib.ptr(xc),
                                    ctypes.byref(xr), _lib.ptr(rowsums.contiguous()), x_layout, N, nb, _lib.ptr(bc),
                                    _lib.ptr(None if out_codes else y), _lib.ptr(y if out_codes else None),
                                    _byref(oq), _lib.ptr(clamped if out_codes else None), _lib.ptr(ws), ws.numel(),
                                    _lib.stream_handle(x.device))
        _lib.check(rc, "packed_igemm")
    if out_codes:
        return QuantizedActivation(y, o3[0], o3[1], o3[2], clamped)
    return y


_opaque_igemm = torch.compiler.disable(_igemm)


def packed_linear_int(xq: QuantizedActivation, p: "PackedTensor", bias: Optional[torch.Tensor] = None,
                      transpose: bool = False, act=None, out_codes: bool = False):
    """``packed_linear`` on activation codes, in integer arithmetic: ``xq.codes [..., K] -> [..., M]``
    (a float tensor, or with ``out_codes=True`` - which needs ``act`` - a ``QuantizedActivation``).
    The weight's row sums are computed on the first call and kept on ``p``."""
    transpose = bool(transpose)
    e = _int_plan(p, transpose, "packed_linear_int")
    o3 = _out_triple(act, out_codes, "packed_linear_int")
    x3 = _in_triple(xq, "packed_linear_int")
    rs = e[2] if e[2] is not None else packed_rowsums(p, transpose)
    return _igemm(p.codes, _meta_words(p), transpose, e[0], e[1], xq.codes, x3, rs, 1, bias, o3, bool(out_codes))


def packed_conv1x1_int(xq: QuantizedActivation, p: "PackedTensor", bias: Optional[torch.Tensor] = None,
                       transpose: bool = False, stride=1, act=None, out_codes: bool = False):
    """``packed_conv1x1`` on activation codes, in integer arithmetic: ``xq.codes [n, K, H, W] ->
    [n, M, H', W']``. The stride sub-samples the code tensor."""
    transpose = bool(transpose)
    e = _int_plan(p, transpose, "packed_conv1x1_int")
    o3 = _out_triple(act, out_codes, "packed_conv1x1_int")
    x3 = _in_triple(xq, "packed_conv1x1_int")
    x = xq.codes
    if x.dim() != 4:
        raise ValueError(f"packed_conv1x1_int: x must be [n, {e[1]}, H, W], got {tuple(x.shape)}")
    if stride != 1:
        sh, sw = (stride, stride) if isinstance(stride, int) else tuple(stride)
        if (sh, sw) != (1, 1):
            x = x[:, :, ::sh, ::sw]
    rs = e[2] if e[2] is not None else packed_rowsums(p, transpose)
    return _igemm(p.codes, _meta_words(p), transpose, e[0], e[1], x, x3, rs, 0, bias, o3, bool(out_codes))


def _pair(v, name: str) -> Tuple[int, int]:
    if isinstance(v, int):
        return v, v
    v = tuple(int(a) for a in v)
    if len(v) != 2:
        raise ValueError(f"{name} must be an int or a pair, got {v}")
    return v


# --- integer fused depthwise + 1x1 ---------------------------------------------
TAPS_MAX = 49   # a 7 x 7 window


def taps_kp(K: int) -> int:
    """Row length of the int8 tap image: ``K`` rounded up to the 64-wide K step."""
    return 64 * ((int(K) + 63) // 64)


def packed_taps_int(C: "PackedTensor") -> torch.Tensor:
    """The int8 image ``[kh kw, Kp]`` (``Kp = taps_kp(K)``) of the packed depthwise factor ``C [kh kw, K]``:
    ``c[tap, k] = (u - q) - zero_point``, columns ``k >= K`` zero (``k_packed_taps_i8``). Kept on ``C``
    while its codes and fields are unchanged, beside the row sums; the host refusals (tensor_minmax, an
    affine record outside int8, more than 49 taps) run once."""
    e = _int_plan(C, False, "packed_taps_int")
    if len(e) < 4:
        if e[0] > TAPS_MAX:
            raise ValueError(f"packed_taps_int: {e[0]} taps are past the limit of {TAPS_MAX} (a 7 x 7 window)")
        e.append(None)
    if e[3] is None:
        if C.codes.device.type != "cuda":
            raise RuntimeError("admmq: packed codes must live on a ROCm GPU (device 'cuda'); the MI355X path has no "
                               "CPU implementation")
        e[3] = _taps_i8(C.codes, _meta_words(C), e[0], e[1])
    return e[3]


@torch.compiler.disable
def _taps_i8(codes, meta_words, ntaps, K):
    if _lib.use_ops():   # torch.ops.admmq.packed_taps_i8 (csrc/torch_ops.cpp) -> admmq_packed_taps_i8
        return _lib.ops().packed_taps_i8(codes, meta_words, ntaps, K)
    cc, meta = _weight_arg(codes, meta_words)
    image = torch.empty((ntaps, taps_kp(K)), dtype=torch.int8, device=cc.device)
    _lib.check(_lib.load().admmq_packed_taps_i8(_lib.ptr(cc), ctypes.byref(meta), ntaps, K, _lib.ptr(image),
                                                _lib.stream_handle(cc.device)), "packed_taps_i8")
    return image


def _idwgemm(codes, meta_words, M, K, x, x3, image, s_c, ks, st, pd, rowsums, bias, m3, o3, out_codes, count_mid=True):
    """The call behind ``packed_depthwise_conv1x1_int`` on checked quantizers ``x3`` / ``m3`` / ``o3 =
    (bits, mn, rng)``: ``(y, mid_clamped, clamped)``, the counters int32 device tensors (``mid_clamped``
    empty without ``count_mid``: the count then costs nothing, not even its memset)."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
        raise TypeError("packed_idwgemm: xq.codes must be a uint8 tensor")
    if bias is not None:
        _inference_only("packed_idwgemm", bias, "bias")
    _require_gpu("packed_idwgemm", "codes, tap image and activations", x, codes, image)
    if torch.compiler.is_compiling():   # opaque under torch.compile, like packed_igemm
        return _opaque_idwgemm(codes, meta_words, M, K, x, x3, image, s_c, ks, st, pd, rowsums, bias, m3, o3, out_codes,
                               count_mid)
    (kh, kw), (sh, sw), (ph, pw) = ks, st, pd
    if bias is not None:
        bias = bias.detach()
    if _lib.use_ops():   # torch.ops.admmq.packed_idwgemm (csrc/torch_ops.cpp) -> admmq_packed_idwgemm
        return _lib.ops().packed_idwgemm(codes, meta_words, M, K, x, x3[0], x3[1], x3[2], image, s_c, kh, kw, sh, sw, ph,
                                         pw, rowsums, bias, m3[0], m3[1], m3[2], o3[0], o3[1], o3[2], out_codes,
                                         bool(count_mid))
    lib = _lib.load()
    _dw_x_shape("packed_idwgemm", x, K)
    if image.dtype != torch.int8 or tuple(image.shape) != (kh * kw, taps_kp(K)):
        raise ValueError(f"packed_idwgemm: the tap image must be int8 [{kh * kw}, {taps_kp(K)}], got {image.dtype} "
                         f"{tuple(image.shape)}")
    if rowsums.dtype != torch.int32 or tuple(rowsums.shape) != (M,):
        raise ValueError(f"packed_idwgemm: rowsums must be int32 [{M}]")
    nb, H, W, Ho, Wo, xc = _dw_geometry("packed_idwgemm", x, ks, st, pd)
    ic = _aligned(image)
    (cc, meta), bc = _weight_arg(codes, meta_words), _bias_arg("packed_idwgemm", bias, M)
    xr, mr, oq = _actq(x3), _actq(m3), _actq(o3)
    y = torch.empty((nb, M, Ho, Wo), dtype=torch.uint8 if out_codes else torch.float32, device=x.device)
    mid_clamped = torch.empty(1 if count_mid else 0, dtype=torch.int32, device=x.device)
    clamped = torch.empty(1 if out_codes else 0, dtype=torch.int32, device=x.device)
    ws = _lib.workspace(lib.admmq_packed_idwgemm_workspace_size(M, K, Ho, Wo, nb), x.device)
    rc = lib.admmq_packed_idwgemm(_lib.ptr(cc), ctypes.byref(meta), M, K, _lib.ptr(xc), ctypes.byref(xr), nb, H, W,
                                  _lib.ptr(ic), s_c, kh, kw, sh, sw, ph, pw, _lib.ptr(rowsums.contiguous()), _lib.ptr(bc),
                                  _lib.ptr(None if out_codes else y), _lib.ptr(y if out_codes else None),
                                  ctypes.byref(mr), _byref(oq), _lib.ptr(mid_clamped if count_mid else None),
                                  _lib.ptr(clamped if out_codes else None), _lib.ptr(ws), ws.numel(),
                                  _lib.stream_handle(x.device))
    _lib.check(rc, "packed_idwgemm")
    return y, mid_clamped, clamped


_opaque_idwgemm = torch.compiler.disable(_idwgemm)


def packed_depthwise_conv1x1_int(xq: QuantizedActivation, C_or_image, p: "PackedTensor", kernel_size=(3, 3), stride=1,
                                 padding=0, bias: Optional[torch.Tensor] = None, mid_act=None, act=None,
                                 out_codes: bool = False, return_mid_clamped: bool = False):
    """``packed_depthwise_conv1x1`` on activation codes, in integer arithmetic from the stencil to the GEMM
    (``k_packed_idwgemm``): ``xq.codes [n, K, H, W] -> [n, M, Ho, Wo]``. ``C_or_image``: the packed depthwise
    factor ``C [kh kw, K]`` (its int8 image is made on the first call and kept on ``C``), or the pair
    ``(packed_taps_int(C), C.scale)``. ``p``: the packed ``A [M, K]``; its row sums are kept on ``p``.
    ``mid_act`` (mandatory, bits 2..8): the quantizer of the depthwise stage's output, whose codes are the
    GEMM's operand. The result is a float tensor (quantized by ``act`` when given) or, with
    ``out_codes=True`` (needs ``act``, bits 2..8), a ``QuantizedActivation`` with its ``clamped`` count on the
    device. ``return_mid_clamped``: return ``(result, mid_clamped)``, the int32 ``[1]`` device count of the
    depthwise outputs whose code was clamped (counted only when asked for: the count costs a memset on the
    stream). No host read. Inference only."""
    who = "packed_depthwise_conv1x1_int"
    e = _int_plan(p, False, who)
    x3 = _in_triple(xq, who)
    mq = _code_act(mid_act, who)
    m3 = (int(mq.bits), float(mq.mn), float(mq.rng))
    o3 = _out_triple(act, out_codes, who)
    ks, st, pd = _pair(kernel_size, "kernel_size"), _pair(stride, "stride"), _pair(padding, "padding")
    if isinstance(C_or_image, PackedTensor):
        if tuple(C_or_image.shape) != (ks[0] * ks[1], e[1]):
            raise ValueError(f"{who}: C must be [{ks[0] * ks[1]}, {e[1]}], got {tuple(C_or_image.shape)}")
        image, s_c = packed_taps_int(C_or_image), float(C_or_image.scale)
    else:
        image, s_c = C_or_image
        s_c = float(s_c)
    rs = e[2] if e[2] is not None else packed_rowsums(p, False)
    y, mid_clamped, clamped = _idwgemm(p.codes, _meta_words(p), e[0], e[1], xq.codes, x3, image, s_c, ks, st, pd, rs, bias,
                                       m3, o3, bool(out_codes), bool(return_mid_clamped))
    res = QuantizedActivation(y, o3[0], o3[1], o3[2], clamped) if out_codes else y
    return (res, mid_clamped) if return_mid_clamped else res


def packed_dwgemm(codes: torch.Tensor, meta_words: torch.Tensor, M: int, K: int, x: torch.Tensor, taps: torch.Tensor,
                  kernel_size, stride=1, padding=0, bias: Optional[torch.Tensor] = None, act=None,
                  mid_act=None) -> torch.Tensor:
    """Depthwise ``kernel_size`` convolution of ``x [n, K, H, W]`` by ``taps [kh kw, K]`` followed by
    the 1x1 convolution by the ``[M, K]`` de-quantization of ``codes`` (+ ``bias``), in one kernel
    (``k_packed_dwgemm``): ``-> [n, M, Ho, Wo]``; the ``K``-channel intermediate is never written.
    ``mid_act`` / ``act = (bits, min_val, max_val)``: fixed-range quantizers of the depthwise stage's
    output (applied as it is staged; padding stays 0) and of the result (``admmq_packed_dwgemm_act``).
    Inference only: an ``x`` that requires grad is refused while grad mode is on."""
    _require_gpu("packed_dwgemm", "codes, taps and activations", x, codes, taps)
    _lib.require_device(x)
    _lib.require_device(taps)
    _inference_only("packed_dwgemm", x, "x")
    if torch.compiler.is_compiling():   # opaque under torch.compile, like packed_gemm
        return _opaque_packed_dwgemm(codes, meta_words, M, K, x, taps, kernel_size, stride, padding, bias, act, mid_act)
    M, K = int(M), int(K)
    ks, st, pd = _pair(kernel_size, "kernel_size"), _pair(stride, "stride"), _pair(padding, "padding")
    (kh, kw), (sh, sw), (ph, pw) = ks, st, pd
    taps = taps.detach()
    if bias is not None:
        bias = bias.detach()
    oq, mq = _act_record(act), _act_record(mid_act)
    if (oq is not None or mq is not None) and _lib.use_ops():   # torch.ops.admmq.packed_dwgemm_act
        m3 = (mq.bits, mq.mn, mq.rng) if mq is not None else (0, 0.0, 0.0)
        o3 = (oq.bits, oq.mn, oq.rng) if oq is not None else (0, 0.0, 0.0)
        return _lib.ops().packed_dwgemm_act(codes, meta_words, M, K, x, taps, kh, kw, sh, sw, ph, pw, bias, *m3, *o3)
    if _lib.use_ops():   # torch.ops.admmq.packed_dwgemm (csrc/torch_ops.cpp) -> admmq_packed_dwgemm
        return _lib.ops().packed_dwgemm(codes, meta_words, M, K, x, taps, kh, kw, sh, sw, ph, pw, bias)
    lib = _lib.load()
    _dw_x_shape("packed_dwgemm", x, K)
    if tuple(taps.shape) != (kh * kw, K):
        raise ValueError(f"packed_dwgemm: taps must be [{kh * kw}, {K}], got {tuple(taps.shape)}")
    nb, H, W, Ho, Wo, xc = _dw_geometry("packed_dwgemm", x, ks, st, pd)
    tc = taps.contiguous()
    (cc, meta), bc = _weight_arg(codes, meta_words), _bias_arg("packed_dwgemm", bias, M)
    y = torch.empty((nb, M, Ho, Wo), dtype=torch.float32, device=x.device)
    ws = _lib.workspace(lib.admmq_packed_dwgemm_workspace_size(M, K, Ho, Wo, nb), x.device)
    if oq is not None or mq is not None:
        rc = lib.admmq_packed_dwgemm_act(_lib.ptr(cc), ctypes.byref(meta), M, K, _lib.ptr(xc), nb, H, W, _lib.ptr(tc), kh,
                                         kw, sh, sw, ph, pw, _lib.ptr(bc), _lib.ptr(y), _byref(mq), _byref(oq),
                                         _lib.ptr(ws), ws.numel(), _lib.stream_handle(x.device))
        _lib.check(rc, "packed_dwgemm_act")
        return y
    rc = lib.admmq_packed_dwgemm(_lib.ptr(cc), ctypes.byref(meta), M, K, _lib.ptr(xc), nb, H, W, _lib.ptr(tc), kh, kw,
                                 sh, sw, ph, pw, _lib.ptr(bc), _lib.ptr(y), _lib.ptr(ws), ws.numel(),
                                 _lib.stream_handle(x.device))
    _lib.check(rc, "packed_dwgemm")
    return y


_opaque_packed_dwgemm = torch.compiler.disable(packed_dwgemm)


def packed_depthwise_conv1x1(x: torch.Tensor, taps: torch.Tensor, p: "PackedTensor",
                             bias: Optional[torch.Tensor] = None, kernel_size=(3, 3), stride=1,
                             padding=0, act=None, mid_act=None) -> torch.Tensor:
    """The last two stages of a 3-way CP layer in one call: ``F.conv2d(z, W[:, :, None, None], bias)`` with
    ``W = p.dequantize()`` (``[M, K]``) and ``z`` the depthwise ``kernel_size`` convolution of ``x [n, K, H, W]``
    (``stride``, zero ``padding``) whose kernel of channel ``k`` is ``taps[:, k]`` (``taps [kh kw, K]``: the
    de-quantized ``C`` factor as it is). ``z`` is formed inside the GEMM's staging and never written; the
    result has the bits of ``packed_conv1x1`` on a ``z`` summed tap by tap in float32. Inference only."""
    M, K = _weight_dims(p, False)
    return packed_dwgemm(p.codes, _meta_words(p), M, K, x, taps, kernel_size, stride, padding, bias, act, mid_act)


def save_packed(path: str, p) -> None:
    """Write one ``PackedTensor`` (or a list of them) as a plain dict of tensors and Python
    scalars; ``load_packed`` reads it back with ``weights_only=True``."""
    many = not isinstance(p, PackedTensor)
    items = [{"codes": q.codes.detach().cpu(), "shape": [int(s) for s in q.shape], "bits": int(q.bits),
              "qscheme": q.qscheme, "scale": float(q.scale), "zero_point": int(q.zero_point), "mn": float(q.mn),
              "rng": float(q.rng), "index": int(q.index)} for q in (p if many else [p])]
    torch.save({"format": FORMAT, "many": many, "tensors": items}, path)


def load_packed(path: str, device=None):
    """The ``PackedTensor`` (or list) ``save_packed`` wrote, with its codes on ``device``."""
    d = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(d, dict) or d.get("format") != FORMAT:
        raise ValueError(f"{path}: not a packed-tensor file ({FORMAT})")
    out = []
    for it in d["tensors"]:
        c = it["codes"]
        if c.dtype != torch.uint8:
            raise TypeError(f"{path}: codes must be uint8, got {c.dtype}")
        out.append(PackedTensor(codes=c.to(device) if device is not None else c, shape=tuple(it["shape"]),
                                bits=int(it["bits"]), qscheme=it["qscheme"], scale=float(it["scale"]),
                                zero_point=int(it["zero_point"]), mn=float(it["mn"]), rng=float(it["rng"]),
                                index=int(it["index"])))
    return out if d["many"] else out[0]


# --- quant + low-rank -----------------------------------------------------------
@dataclass
class PackedLowRank:
    """``W ~ W_q + W_r`` of ``admmq.lowrank`` in its deployable form: ``q`` the packed codes of ``W_q [M, K]``,
    ``L [M, r]`` and ``Rt [r, K]`` the float32 factors of ``W_r = L Rt`` (``K`` contiguous in ``Rt``: the
    down-projection streams along it)."""
    q: PackedTensor
    L: torch.Tensor
    Rt: torch.Tensor

    @property
    def rank(self) -> int:
        return int(self.L.shape[1])

    @property
    def nbytes(self) -> int:
        """Resident bytes of the weights: the code stream and the two factors."""
        return self.q.nbytes + 4 * (int(self.L.numel()) + int(self.Rt.numel()))

    def dequantize(self) -> torch.Tensor:
        """``W_q + L Rt`` as a float32 ``[M, K]`` tensor (the library product; for comparisons)."""
        return self.q.dequantize() + self.L @ self.Rt


def _lowrank_dims(p: "PackedLowRank") -> Tuple[int, int, int]:
    """``(M, K, r)`` of ``p``, checked on the host."""
    if not isinstance(p, PackedLowRank):
        raise TypeError("expected a PackedLowRank")
    M, K = _weight_dims(p.q, False)
    L, Rt = p.L, p.Rt
    if L.dim() != 2 or Rt.dim() != 2 or L.shape[0] != M or Rt.shape[1] != K or L.shape[1] != Rt.shape[0]:
        raise ValueError(f"PackedLowRank: L must be [{M}, r] and Rt [r, {K}], got {tuple(L.shape)} and {tuple(Rt.shape)}")
    if L.dtype != torch.float32 or Rt.dtype != torch.float32:
        raise TypeError(f"PackedLowRank: L and Rt must be float32, got {L.dtype} and {Rt.dtype}")
    r = int(L.shape[1])
    if not 1 <= r <= RANK_MAX:
        raise ValueError(f"PackedLowRank: rank must be 1..{RANK_MAX}, got {r}")
    return M, K, r


def packed_lrgemm(codes: torch.Tensor, meta_words: torch.Tensor, M: int, K: int, L: torch.Tensor, Rt: torch.Tensor,
                  x: torch.Tensor, bias: Optional[torch.Tensor] = None, out_dtype=None) -> torch.Tensor:
    """``y = x (D + L Rt)^T (+ bias)`` with ``D`` the ``[M, K]`` de-quantization of ``codes``, ``L [M, r]`` and
    ``Rt [r, K]`` float32 (``admmq_packed_lrgemm``): ``x [..., K] -> [..., M]``. Neither ``D`` nor ``L Rt`` is
    written to memory. A bfloat16 / float16 ``x`` is a composition, not a fused kernel:
    ``(packed_gemm(x, out float32) + (x.float() @ Rt.float().T) @ L.float().T + bias)`` converted once to ``x``'s
    dtype (or kept float32 with ``out_dtype=torch.float32``); ``L`` / ``Rt`` / ``bias`` may then be of ``x``'s dtype
    (a module after ``.half()``). Inference only: an ``x`` that requires grad is refused while grad mode is on."""
    _require_gpu("packed_lrgemm", "codes, factors and activations", x, codes, L, Rt)
    if x.dtype in HALF_DTYPES:
        if out_dtype is not None and out_dtype != torch.float32 and out_dtype != x.dtype:
            raise ValueError(f"packed_lrgemm: out_dtype must be None, torch.float32 or x's dtype {x.dtype}, got {out_dtype}")
        y = packed_gemm(codes, meta_words, False, M, K, x, 1, None, None, torch.float32)
        y = y + (x.detach().float() @ Rt.detach().float().T) @ L.detach().float().T
        if bias is not None:
            y = y + bias.detach().float()
        return y if out_dtype == torch.float32 else y.to(x.dtype)
    if out_dtype is not None and out_dtype != torch.float32:
        raise ValueError(f"packed_lrgemm: a float32 x gives a float32 result, not out_dtype={out_dtype}")
    _lib.require_device(x)
    _inference_only("packed_lrgemm", x, "x")
    if torch.compiler.is_compiling():   # opaque under torch.compile, like packed_gemm
        return _opaque_packed_lrgemm(codes, meta_words, M, K, L, Rt, x, bias)
    M, K = int(M), int(K)
    L, Rt = L.detach(), Rt.detach()
    if bias is not None:
        bias = bias.detach()
    if _lib.use_ops():   # torch.ops.admmq.packed_lrgemm (csrc/torch_ops.cpp) -> admmq_packed_lrgemm
        return _lib.ops().packed_lrgemm(codes, meta_words, M, K, L, Rt, x, bias)
    lib = _lib.load()
    _lib.require_device(L)
    _lib.require_device(Rt)
    if L.dim() != 2 or Rt.dim() != 2 or L.shape[0] != M or Rt.shape[1] != K or L.shape[1] != Rt.shape[0]:
        raise ValueError(f"packed_lrgemm: L must be [{M}, r] and Rt [r, {K}], got {tuple(L.shape)} and {tuple(Rt.shape)}")
    oshape, _, N, xc = _gemm_geometry("packed_lrgemm", x, M, K, 1)
    Lc, Rc, r = L.contiguous(), Rt.contiguous(), int(L.shape[1])
    (cc, meta), bc = _weight_arg(codes, meta_words), _bias_arg("packed_lrgemm", bias, M)
    y = torch.empty(oshape, dtype=torch.float32, device=x.device)
    ws = _lib.workspace(lib.admmq_packed_lrgemm_workspace_size(M, K, N, r), x.device)
    rc = lib.admmq_packed_lrgemm(_lib.ptr(cc), ctypes.byref(meta), M, K, _lib.ptr(Lc), _lib.ptr(Rc), r, _lib.ptr(xc), N,
                                 _lib.ptr(bc), _lib.ptr(y), _lib.ptr(ws), ws.numel(), _lib.stream_handle(x.device))
    _lib.check(rc, "packed_lrgemm")
    return y


_opaque_packed_lrgemm = torch.compiler.disable(packed_lrgemm)


def packed_lowrank_linear(x: torch.Tensor, p: "PackedLowRank", bias: Optional[torch.Tensor] = None,
                          out_dtype=None) -> torch.Tensor:
    """``F.linear(x, W_q + L Rt, bias)`` computed from ``p``'s codes and factors in one GEMM: ``x [..., K] ->
    [..., M]``. A bfloat16 / float16 ``x`` runs ``packed_lrgemm``'s composition (the half packed GEMM plus two
    library products in float32; not a fused kernel). Inference only."""
    M, K, _ = _lowrank_dims(p)
    return packed_lrgemm(p.q.codes, _meta_words(p.q), M, K, p.L, p.Rt, x, bias, out_dtype)


def save_packed_lowrank(path: str, p: "PackedLowRank") -> None:
    """Write a ``PackedLowRank`` as a plain dict of tensors and Python scalars; ``load_packed_lowrank`` reads it
    back with ``weights_only=True``."""
    _lowrank_dims(p)
    q = p.q
    torch.save({"format": FORMAT_LOWRANK,
                "q": {"codes": q.codes.detach().cpu(), "shape": [int(s) for s in q.shape], "bits": int(q.bits),
                      "qscheme": q.qscheme, "scale": float(q.scale), "zero_point": int(q.zero_point), "mn": float(q.mn),
                      "rng": float(q.rng), "index": int(q.index)},
                "L": p.L.detach().cpu().contiguous(), "Rt": p.Rt.detach().cpu().contiguous()}, path)


def load_packed_lowrank(path: str, device=None) -> "PackedLowRank":
    """The ``PackedLowRank`` that ``save_packed_lowrank`` wrote, with its tensors on ``device``."""
    d = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(d, dict) or d.get("format") != FORMAT_LOWRANK:
        raise ValueError(f"{path}: not a packed quant + low-rank file ({FORMAT_LOWRANK})")
    it = d["q"]
    c = it["codes"]
    if c.dtype != torch.uint8:
        raise TypeError(f"{path}: codes must be uint8, got {c.dtype}")
    to = (lambda t: t.to(device)) if device is not None else (lambda t: t)
    p = PackedLowRank(q=PackedTensor(codes=to(c), shape=tuple(it["shape"]), bits=int(it["bits"]), qscheme=it["qscheme"],
                                     scale=float(it["scale"]), zero_point=int(it["zero_point"]), mn=float(it["mn"]),
                                     rng=float(it["rng"]), index=int(it["index"])),
                      L=to(d["L"]), Rt=to(d["Rt"]))
    _lowrank_dims(p)
    return p
