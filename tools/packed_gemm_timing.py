#!/usr/bin/env python3
"""Timing of the packed-weight GEMM against the routes that go through a
float32 weight, on the MI355X. Writes profiles/packed_gemm_timing.json's "calls_us" part.

Routes, alternating within one job (two rounds):
  fused     packed_conv1x1 / packed_linear: one call, the codes are decoded in the GEMM
  dequant   dequantize_packed followed by F.conv2d / F.linear on its result (both timed
            together): the only route from packed codes before the fused kernel
  resident  F.conv2d / F.linear on an already resident float32 weight (8x the memory at 4 bits)
Method: HIP events around `reps` back-to-back calls, 10 warm-up calls, `samples` samples,
median [p10, p90] in microseconds per call.
  --trace   few calls per route, for a `rocprofv3 --kernel-trace` run of its own
  --kernels DIR   read that run's kernel_trace.csv and add "kernels_us" to the JSON
usage: packed_gemm_timing.py --out FILE [--samples 40] [--trace] [--kernels DIR]"""
import argparse
import collections
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))

BITS, SCHEME = 4, "tensor_mseminmax_symmetric"
# (name, kind, packed shape, transpose, [(label, activations shape)])
CASES = [
    ("layer4_conv1_M1141_K512_T", "conv", (512, 1141), True, [("N49", (1, 512, 7, 7)), ("N3136", (64, 512, 7, 7))]),
    ("layer4_conv3_M512_K1141", "conv", (512, 1141), False, [("N49", (1, 1141, 7, 7)), ("N3136", (64, 1141, 7, 7))]),
    ("c5_linear_M4096_K1024", "linear", (4096, 1024), False,
     [("tok1", (1, 1024)), ("tok16", (16, 1024)), ("tok512", (512, 1024))]),
]


def pieces(K):
    kp = max(64, 32 * ((K + 1023) // 1024))
    return (K + kp - 1) // kp


def grid_of(M, K, C):
    """k_packed_gemm's launch grid in threads (the planner's rule, packed_gemm.hip)."""
    tm, tc, np_ = (M + 63) // 64, (C + 63) // 64, pieces(K)
    par = np_ > 1 and tm * tc < 256
    return [tc * 256, tm, np_ if par else 1]


def kernels(trace_dir):
    f = glob.glob(f"{trace_dir}/**/*kernel_trace.csv", recursive=True)[0]
    d = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        n = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("admmq::", "")
        key = f"{n[:60]} grid {r['Grid_Size_X']}x{r['Grid_Size_Y']}x{r['Grid_Size_Z']}"
        d[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for k, v in sorted(d.items()):
        v.sort()
        if len(v) >= 5:
            out[k] = {"launches": len(v), "median": round(v[len(v) // 2], 2), "min": round(v[0], 2)}
    return out


def main():
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
    from admmq import packed_conv1x1, packed_linear, quantize_packed
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "grids": {}, "check_rel": {}}
    for name, kind, shape, tr, acts in CASES:
        p = quantize_packed([(torch.randn(*shape, generator=g) * 0.05).to(dev)], BITS, SCHEME)[0]
        D = p.dequantize()
        Wres = (D.T if tr else D).contiguous()
        M, K = Wres.shape
        for label, xs in acts:
            x = torch.randn(*xs, generator=g).to(dev)
            C = x.numel() // K
            if kind == "conv":
                routes = {
                    "fused": lambda: packed_conv1x1(x, p, transpose=tr),
                    "dequant": lambda: F.conv2d(x, (p.dequantize().T if tr else p.dequantize())[:, :, None, None]),
                    "resident": lambda: F.conv2d(x, Wres[:, :, None, None]),
                }
            else:
                routes = {
                    "fused": lambda: packed_linear(x, p, transpose=tr),
                    "dequant": lambda: F.linear(x, p.dequantize().T if tr else p.dequantize()),
                    "resident": lambda: F.linear(x, Wres),
                }
            key = f"{name}_{label}"
            res["grids"][key] = grid_of(M, K, C)
            y, yr = routes["fused"](), routes["resident"]()
            res["check_rel"][key] = float((y - yr).norm() / yr.norm())
            reps = 4 if C > 256 else 20
            nsamp = 3 if args.trace else args.samples
            out = res["calls_us"][key] = {}
            with torch.no_grad():
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
            print(key, json.dumps(out), flush=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
