#!/usr/bin/env python3
"""Timing of the integer fused depthwise + 1x1 stage and of the 3-way integer CP layer
 against the float fused route they stand beside, on the MI355X, on DESIGN.md
2.23's three shapes with 4-bit weights, 8-bit codes and all quantizers on. Writes
profiles/packed_icp_timing.json.

Stage routes, alternating within one job (two rounds); both start from conv1's output:
  integer   packed_depthwise_conv1x1_int: t's codes in (encoded before the timed region), mid and
            output quantizer on, float out; row sums and tap image on the packed tensors before
            the first sample
  integer_counted   the same call with return_mid_clamped=True: the clamp counter of Z costs one
            more submission (its memset on the stream)
  fused     packed_depthwise_conv1x1 on the float t with the same mid and output quantizers
            (k_packed_dwgemm<.., QM>)
Layer routes ("layers_us"): build_cp_layer(integer=True) against build_cp_layer(fused=True,
act_quant=...) on the float input, cin = M.
Method: HIP events around `reps` back-to-back calls, 10 warm-up calls, `samples` samples,
median [p10, p90] in microseconds per call. "goals": at the two nb = 1 shapes the integer
stage's median (the mean of its two rounds' medians) may exceed the fused stage's by no more
than the larger of the two routes' round-to-round spreads; nb = 64 is reported without one.
  --trace   few calls per route, for a `rocprofv3 --kernel-trace --stats` run of its own
  --kernels DIR   read that run's kernel_trace.csv and add "kernels_us" to the JSON
usage: packed_icp_timing.py --out FILE [--samples 40] [--trace] [--kernels DIR]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from packed_cp_timing import BITS, CASES, SCHEME   # noqa: E402  (2.23's three shapes)
from packed_igemm_timing import rounds             # noqa: E402  (the same sampling)

XACT = (8, -4.0, 4.0)


def main():
    from packed_gemm_timing import grid_of, kernels
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernels", default=None)
    args = ap.parse_args()
    if args.kernels:
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        res["kernels_us"] = kernels(args.kernels)
        json.dump(res, open(args.out, "w"), indent=1)
        return
    import torch
    import torch.nn.functional as F
    from admmq import (act_encode, export, packed_depthwise_conv1x1, packed_depthwise_conv1x1_int, packed_rowsums,
                       packed_taps_int, quantize_packed)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    nsamp = 3 if args.trace else args.samples
    res = {"calls_us": {}, "grids": {}, "check_rel": {}, "clamped": {}, "goals": {}, "layers_us": {}}
    with torch.no_grad():
        for name, M, R, (H, W), k, pad, stride, nb in CASES:
            A, B, C = quantize_packed([(torch.randn(M, R, generator=g) * 0.05).to(dev),
                                       (torch.randn(M, R, generator=g) * 0.05).to(dev),
                                       (torch.randn(k * k, R, generator=g) * 0.3).to(dev)], BITS, SCHEME)
            taps = C.dequantize()
            bias = torch.randn(M, generator=g).to(dev)
            t = torch.randn(nb, R, H, W, generator=g).clamp_(-3.9, 3.9).to(dev)
            z = F.conv2d(t, taps.reshape(k, k, R).permute(2, 0, 1)[:, None].contiguous(), None, stride, pad, 1, R)
            y0 = F.conv2d(z, A.dequantize()[:, :, None, None], bias)
            mid = (8, float(z.min()) - 0.05, float(z.max()) + 0.05)
            out = (8, float(y0.min()) - 0.05, float(y0.max()) + 0.05)
            del z, y0
            tq = act_encode(t, XACT)
            packed_rowsums(A), packed_taps_int(C)
            routes = {
                "integer": lambda: packed_depthwise_conv1x1_int(tq, C, A, (k, k), stride, pad, bias, mid, out),
                "integer_counted": lambda: packed_depthwise_conv1x1_int(tq, C, A, (k, k), stride, pad, bias, mid, out,
                                                                        return_mid_clamped=True),
                "fused": lambda: packed_depthwise_conv1x1(t, taps, A, bias, (k, k), stride, pad, out, mid),
            }
            Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
            cols = nb * Ho * Wo
            res["grids"][name] = grid_of(M, R, cols)
            yi, mc = packed_depthwise_conv1x1_int(tq, C, A, (k, k), stride, pad, bias, mid, out, return_mid_clamped=True)
            yf = routes["fused"]()
            res["check_rel"][name] = float((yi - yf).norm() / yf.norm())   # (t's 8-bit quantization)
            res["clamped"][name] = int(mc)
            reps = 4 if cols > 256 else 20
            o = res["calls_us"][name] = rounds(routes, reps, nsamp)
            ig, fu = [o[f"integer_run{r}"][0] for r in (1, 2)], [o[f"fused_run{r}"][0] for r in (1, 2)]
            spread = max(abs(ig[0] - ig[1]), abs(fu[0] - fu[1]))
            mi, mf = sum(ig) / 2, sum(fu) / 2
            res["goals"][name] = {"integer": round(mi, 2), "fused": round(mf, 2), "round_spread": round(spread, 1),
                                  "integer_counted": round(sum(o[f"integer_counted_run{r}"][0] for r in (1, 2)) / 2, 2)}
            if nb == 1:
                res["goals"][name].update(kind="not above fused by more than the spread", met=bool(mi <= mf + spread),
                                          met_worst_round=bool(max(ig) <= min(fu) + spread))
            else:
                res["goals"][name].update(kind="reported without a threshold")
            print(name, json.dumps(o), json.dumps(res["goals"][name]), flush=True)
            # the whole layer: cin = M, the float input x -> conv1 -> the stage
            x = torch.randn(nb, M, H, W, generator=g).clamp_(-3.9, 3.9).to(dev)
            plain = export.build_cp_layer(R, [A, B, C], bias, M, M, (k, k), pad, stride, fused=True)
            h = plain.conv1(x)
            acts = [(8, float(h.min()) - 0.05, float(h.max()) + 0.05), mid, out]
            del h
            fl = export.build_cp_layer(R, [A, B, C], bias, M, M, (k, k), pad, stride, fused=True, act_quant=acts)
            il = export.build_cp_layer(R, [A, B, C], bias, M, M, (k, k), pad, stride, act_quant=acts, integer=True,
                                       in_act=XACT)
            res["layers_us"][name] = rounds({"integer": lambda: il(x), "fused": lambda: fl(x)}, reps, nsamp)
            res["layers_us"][name]["rel_integer_vs_fused"] = float((il(x) - fl(x)).norm() / fl(x).norm())
            print("layer", name, json.dumps(res["layers_us"][name]), flush=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
