"""Activation-quantization modules (``source/quantization.py:168-298``) on the MI355X.

``FixedQuant`` quantizes to a range given at construction; ``MinMaxQuant`` and
``MovingAvgMinMaxQuant`` first observe ``counter`` samples (running min / max, or their moving
average) and quantize with the observed range from then on. They keep the reference's
constructor arguments, ``counter`` property, ``repr`` and the ``activation_post_process`` layout
of ``add_quant``. The statistics are 0-dim float32 tensors on the input's device, updated with
the reference's float32 expressions: observing never synchronises with the host. The first
quantizing forward reads them once (one sync) and keeps the ``(mn, rng)`` pair; the
quantization itself is ``k_fixed_quant`` (``admmq.min_max_quantize``). Inference only.

``collect(seq)`` reads the calibrated ranges of a layer whose stages were wrapped by
``add_quant``, in the form the ``admmq.export`` builders take as ``act_quant=``.
"""
from __future__ import annotations

from collections import OrderedDict

import torch
from torch import nn

from .quantization import _fixed, act_range, fixed_quantize

__all__ = ["FixedQuant", "MinMaxQuant", "MovingAvgMinMaxQuant", "get_quant_layer", "add_quant", "collect"]


class FixedQuant(nn.Module):
    """``fixed_quantize(x, bits, zero_point, scope)``; the identity while either is ``None``."""

    def __init__(self, name, bits, **kwargs):
        super().__init__()
        self.name, self.bits = name, bits
        self.quant_func = fixed_quantize
        self.zero_point, self.scope = kwargs['zero_point'], kwargs['scope']
        self.min_max = kwargs.get('min_max')   # the (min, max) the range was made from, where known (collect)

    def forward(self, x_orig):
        if self.zero_point is None or self.scope is None:
            return x_orig
        return self.quant_func(x_orig, self.bits, self.zero_point, self.scope)

    def __repr__(self):
        return f'{type(self).__name__}(bits={self.bits} zero_point={self.zero_point} scope={self.scope})'


class _RangeObserver(nn.Module):
    """Observe while ``counter > 0`` (it falls by the batch length per call), quantize afterwards."""

    def __init__(self, name, bits, counter, **kwargs):
        super().__init__()
        self.name, self.bits = name, bits
        self.quant_func = _fixed
        self._counter = counter
        self.min_val = None
        self.max_val = None
        self._range = None   # (mn, rng) read from the statistics by the first quantizing forward

    @property
    def counter(self):
        return self._counter

    def _merge(self, lo, hi):
        raise NotImplementedError

    def forward(self, x_orig):
        if self._counter > 0:
            self._counter -= len(x_orig)
            if x_orig.numel() == 0:
                return x_orig
            lo, hi = torch.aminmax(x_orig.detach())
            if self.min_val is None or self.max_val is None:
                self.min_val, self.max_val = lo.to(torch.float).clone(), hi.to(torch.float).clone()
            else:
                self._merge(lo, hi)
            self._range = None
            return x_orig
        if self._range is None:
            if self.min_val is None or self.max_val is None:
                raise RuntimeError(f"{self.name}: quantizing before any batch was observed")
            self._range = act_range(self.min_val, self.max_val)   # the one host read
        return self.quant_func(x_orig, self.bits, *self._range)

    def __repr__(self):
        return f'{type(self).__name__}(bits={self.bits} min_val={self.min_val} max_val={self.max_val})'


class MinMaxQuant(_RangeObserver):
    """Running minimum and maximum over the observed batches."""

    def _merge(self, lo, hi):
        self.min_val.copy_(torch.min(lo, self.min_val))
        self.max_val.copy_(torch.max(hi, self.max_val))


class MovingAvgMinMaxQuant(_RangeObserver):
    """Moving average of the batches' minimum and maximum (``averaging_constant`` 0.01)."""

    def __init__(self, name, bits, counter, **kwargs):
        super().__init__(name, bits, counter, **kwargs)
        self.averaging_constant = 0.01

    def _merge(self, lo, hi):
        c = self.averaging_constant
        self.min_val.copy_(self.min_val + c * (lo - self.min_val))
        self.max_val.copy_(self.max_val + c * (hi - self.max_val))


_LAYERS = {'minmax': MinMaxQuant, 'avgminmax': MovingAvgMinMaxQuant, 'fixed': FixedQuant}


def get_quant_layer(ltype, name, **kwargs):
    if ltype == 'histogram':
        raise NotImplementedError("histogram: the observer's range search is a host loop over 2048 bins per batch; "
                                  "it is not part of the device path (its quantizing phase is min_max_quantize)")
    if ltype not in _LAYERS:
        raise NotImplementedError(ltype)
    return _LAYERS[ltype](f'{name}_quant', **kwargs)


def add_quant(name, module, ltype, **kwargs):
    """``module`` followed by its quantizer as ``activation_post_process``; the children of an
    ``nn.Sequential`` are taken over under their own names."""
    parts = OrderedDict(module.named_children()) if isinstance(module, nn.Sequential) else OrderedDict([(name, module)])
    parts['activation_post_process'] = get_quant_layer(ltype, name, **kwargs)
    return nn.Sequential(parts)


def collect(seq):
    """Per stage of ``seq`` in order: ``(bits, min_val, max_val)`` as Python numbers where the stage
    was wrapped by ``add_quant`` and has a range (calibrated, or fixed with a known min / max),
    else ``None``. Reading a device statistic synchronises once per stage."""
    out = []
    for stage in seq.children():
        q = getattr(stage, 'activation_post_process', None) if isinstance(stage, nn.Sequential) else None
        if isinstance(q, _RangeObserver) and q.min_val is not None and q.max_val is not None:
            out.append((int(q.bits), float(q.min_val), float(q.max_val)))
        elif isinstance(q, FixedQuant) and q.min_max is not None:
            out.append((int(q.bits), float(q.min_max[0]), float(q.min_max[1])))
        else:
            out.append(None)
    return out
