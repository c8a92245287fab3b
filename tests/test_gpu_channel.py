"""GPU parity of the per-channel quantizer (k_channel_stats / k_channel_quant, C-ABI
admmq_quantize_channel) past its fixture shapes, against oracle.quant_oracle.quantize_channel
(pinned to the reference by F9, tests/test_oracle_golden.py): bit-equal values and shape.

The F9 KATs stop at 64 x 134, where a channel fits one block. These shapes split a channel
over several blocks (channels above 16384 elements), so the {~min, max, nan} words are
merged across blocks by atomicMax, and they run the 2048 / C cap on the blocks per
channel, the B == 1 strided read and the C == 1 / L == 1 broadcasts above one block:

  (40000, 3)    dim 1, -1   B = 1 strided read, 3 blocks per channel
  (5, 20000, 5) dim 0       7 blocks per channel
  (1, 50000)    dim 0       C = 1: one channel's statistics for every column, 4 blocks
  (40, 2000, 40) dim 2      5 blocks per channel
  (1500, 1)     dim 0       cap: one block per channel, 1500 stats blocks; L = 1 broadcasts
                            to a 1500 x 1500 output
  (40000, 3) with a NaN in channel 1 and +inf / -inf in channel 2, in rows past 16384 that
  different blocks read: the flag and the extremes cross blocks.

NaNs compare as NaNs (payload and sign canonicalised, as gc.canonical_sha does). Signed
zeros are left out: numpy's max of +0 / -0 is not defined.
"""
import functools

import numpy as np
import pytest

from conftest import gpu_available
from oracle import quant_oracle as qo

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SCHEMES = ("channel_symmetric", "channel_affine")
BITS = (2, 4, 8)

# id -> (shape, dim, special values)
CASES = {
    "40000x3_d1": ((40000, 3), 1, False),
    "40000x3_dm1": ((40000, 3), -1, False),
    "5x20000x5_d0": ((5, 20000, 5), 0, False),
    "1x50000_d0": ((1, 50000), 0, False),
    "40x2000x40_d2": ((40, 2000, 40), 2, False),
    "1500x1_d0": ((1500, 1), 0, False),
    "40000x3_d1_special": ((40000, 3), 1, True),
}


@functools.lru_cache(maxsize=None)
def _input(cid):
    shape, _, special = CASES[cid]
    g = np.random.default_rng(90 + list(CASES).index(cid))
    x = (g.standard_normal(shape) * 0.7).astype(np.float32)
    if special:   # with 3 blocks per channel, block (row // 256) % 3 reads the row
        x[30000, 1] = np.nan     # block 0
        x[20000, 2] = np.inf     # block 0
        x[35000, 2] = -np.inf    # block 1
    return x


@functools.lru_cache(maxsize=None)
def _want(cid, bits, qs):
    return _canon(qo.quantize_channel(_input(cid), bits, qs, CASES[cid][1]))


def _canon(a):
    a = np.ascontiguousarray(a, dtype=np.float32).copy()
    u = a.view(np.uint32)
    u[np.isnan(a)] = np.uint32(0x7FC00000)
    return u


@pytest.mark.parametrize("route", ["ops", "cabi"])
@pytest.mark.parametrize("cid", list(CASES))
def test_channel_quantizer_multi_block(cid, route, monkeypatch):
    import torch
    from admmq import _lib, quantize_tensor
    if route == "cabi":
        monkeypatch.setattr(_lib, "use_ops", lambda: False)
    dim = CASES[cid][1]
    x = torch.from_numpy(_input(cid).copy()).to("cuda:0")
    bad = []
    for qs in SCHEMES:
        for bits in BITS:
            want = _want(cid, bits, qs)
            y = quantize_tensor(x, bits, qs, dim=dim)
            assert tuple(y.shape) == want.shape, (qs, bits, tuple(y.shape), want.shape)
            got = _canon(y.cpu().numpy())
            if not np.array_equal(got, want):
                bad.append((qs, bits, int(np.count_nonzero(got != want))))
    assert bad == [], f"(scheme, bits, differing elements): {bad}"
    if CASES[cid][2]:   # the special values reached the statistics
        w = _want(cid, 4, "channel_symmetric").view(np.float32)
        assert np.isnan(w[:, 1]).all() and np.isfinite(w[:, 0]).all()
