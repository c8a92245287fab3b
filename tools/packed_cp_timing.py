#!/usr/bin/env python3
"""Timing of the fused depthwise + 1x1 stage of a packed CP layer against the
two routes it replaces, on the MI355X. Writes profiles/packed_cp_timing.json's "calls_us" part.

Routes, alternating within one job (two rounds); all start from conv1's output t [nb, R, H, W]:
  fused     packed_depthwise_conv1x1: one call, Z is formed inside the GEMM's staging
  unfused   nn.Conv2d depthwise (conv2) followed by PackedConv1x1 (conv3): the packed layer's
            conv2 / conv3 without the fused stage
  float     F.conv2d depthwise + F.conv2d 1x1 on resident float32 weights
Method: HIP events around `reps` back-to-back calls, 10 warm-up calls, `samples` samples,
median [p10, p90] in microseconds per call. "requirement": in the weight-bound case (layer4,
nb = 1) the fused median may exceed the unfused median by no more than the spread between the
two rounds of a route in that job.
  --trace   few calls per route, for a `rocprofv3 --kernel-trace --stats` run of its own
  --kernels DIR   read that run's kernel_trace.csv and add "kernels_us" to the JSON
usage: packed_cp_timing.py --out FILE [--samples 40] [--trace] [--kernels DIR]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BITS, SCHEME = 4, "tensor_mseminmax_symmetric"
# (name, M, R, (H, W), k, pad, stride, nb)
CASES = [
    ("layer4_tail_M512_R1141_7x7_nb1", 512, 1141, (7, 7), 3, 1, 1, 1),
    ("layer4_tail_M512_R1141_7x7_nb64", 512, 1141, (7, 7), 3, 1, 1, 64),
    ("layer2_down_M128_R286_56x56_s2_nb1", 128, 286, (56, 56), 3, 1, 2, 1),
]
WEIGHT_BOUND = CASES[0][0]


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
    from torch import nn
    from admmq import packed_conv1x1, packed_depthwise_conv1x1, quantize_packed
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "grids": {}, "check_rel": {}, "bytes": {}, "flops": {}}
    for name, M, R, (H, W), k, pad, stride, nb in CASES:
        A, C = quantize_packed([(torch.randn(M, R, generator=g) * 0.05).to(dev),
                                (torch.randn(k * k, R, generator=g) * 0.3).to(dev)], BITS, SCHEME)
        taps = C.dequantize()
        Wa = A.dequantize()[:, :, None, None].contiguous()
        Wc = taps.reshape(k, k, R).permute(2, 0, 1)[:, None].contiguous()
        conv2 = nn.Conv2d(R, R, k, groups=R, padding=pad, stride=stride, bias=False, device=dev)
        conv2.weight = nn.Parameter(Wc, requires_grad=False)
        bias = torch.randn(M, generator=g).to(dev)
        t = torch.randn(nb, R, H, W, generator=g).to(dev)
        routes = {
            "fused": lambda: packed_depthwise_conv1x1(t, taps, A, bias, (k, k), stride, pad),
            "unfused": lambda: packed_conv1x1(conv2(t), A, bias),
            "float": lambda: F.conv2d(F.conv2d(t, Wc, None, stride, pad, 1, R), Wa, bias),
        }
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        cols = nb * Ho * Wo
        res["grids"][name] = grid_of(M, R, cols)
        # the fused call's compulsory traffic (codes + t + taps + y) and its GEMM work
        res["bytes"][name] = A.nbytes + 4 * (t.numel() + taps.numel() + M * cols)
        res["flops"][name] = 2 * M * R * cols
        with torch.no_grad():
            y, yu, yf = routes["fused"](), routes["unfused"](), routes["float"]()
            res["check_rel"][name] = {"fused_vs_unfused": float((y - yu).norm() / yu.norm()),
                                      "fused_vs_float": float((y - yf).norm() / yf.norm())}
            reps = 4 if cols > 256 else 20
            nsamp = 3 if args.trace else args.samples
            out = res["calls_us"][name] = {}
            for rnd in (1, 2):
                for rname, fn in routes.items():
                    for _ in range(10):
                        fn()
                    ts = []
                    for _ in range(nsamp):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(reps):
                            fn()
                        e1.record()
                        e1.synchronize()
                        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
                    ts.sort()
                    out[f"{rname}_run{rnd}"] = [round(ts[len(ts) // 2], 1), round(ts[len(ts) // 10], 1),
                                                round(ts[(9 * len(ts)) // 10], 1)]
        print(name, json.dumps(out), flush=True)
    c = res["calls_us"][WEIGHT_BOUND]
    med = {r: sorted(c[f"{r}_run{n}"][0] for n in (1, 2)) for r in ("fused", "unfused", "float")}
    spread = max(med[r][1] - med[r][0] for r in ("fused", "unfused"))
    fused, unfused = sum(med["fused"]) / 2, sum(med["unfused"]) / 2
    res["requirement"] = {"case": WEIGHT_BOUND, "fused_us": fused, "unfused_us": unfused, "round_spread_us": round(spread, 1),
                          "met": bool(fused <= unfused + spread)}
    print("requirement", json.dumps(res["requirement"]), flush=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
