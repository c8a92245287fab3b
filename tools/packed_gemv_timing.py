#!/usr/bin/env python3
"""Timing of the skinny packed GEMV on the MI355X against the route a user had
before it and against a dense weight. Writes profiles/packed_gemv_timing.json.

Routes, alternating within one job (two rounds), for float32 and bfloat16 activations at 4 bits,
1 / 4 / 8 tokens:
  gemv      packed_linear(x, p, skinny=True): k_packed_gemv / k_packed_gemv_t
  gemm      packed_linear(x, p): today's 64 x 64 MFMA tile route, the yardstick
  resident  F.linear on a resident dense weight of x's dtype (context only)
For gemv also the code stream's bytes per second of the median and their share of the data-sheet
HBM bandwidth (8 TB/s). The times are per call from Python, back to back on one stream: they hold
the call's host cost, which all three routes pay.
Cases: the linear shapes of DESIGN.md 2.29, and 4096 x 4096 in the D^T orientation.
Method (tools/packed_hgemm_timing.py's): HIP events around `reps` back-to-back calls, 10 warm-up
calls, `samples` samples, median [p10, p90] in microseconds per call.
usage: packed_gemv_timing.py --out FILE [--samples 20] [--only SUBSTR]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))

BITS, SCHEME = 4, "tensor_mseminmax_symmetric"
HBM_BYTES_PER_S = 8.0e12
TOKENS = [1, 4, 8]
# (name, packed shape, transpose)
CASES = [
    ("c5_linear_M4096_K1024", (4096, 1024), False),
    ("llama_M4096_K4096", (4096, 4096), False),
    ("llama_M4096_K4096_T", (4096, 4096), True),
    ("llama_M11008_K4096", (11008, 4096), False),
    ("llama_M4096_K11008", (4096, 11008), False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from admmq import packed_linear, quantize_packed
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "check_rel": {}, "gemv_stream": {},
           "method": "median [p10, p90] us per call; two alternating rounds; stream: code bytes / median, share of 8 TB/s"}
    for name, shape, tr in CASES:
        if args.only and args.only not in name:
            continue
        p = quantize_packed([(torch.randn(*shape, generator=g) * 0.05).to(dev)], BITS, SCHEME)[0]
        D = p.dequantize()
        K = (D.T if tr else D).shape[1]
        for dtype, dname in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
            Wres = (D.T if tr else D).contiguous().to(dtype)
            for tok in TOKENS:
                x = torch.randn(tok, K, generator=g).to(dev).to(dtype)
                routes = {
                    "gemv": lambda: packed_linear(x, p, transpose=tr, skinny=True),
                    "gemm": lambda: packed_linear(x, p, transpose=tr),
                    "resident": lambda: F.linear(x, Wres),
                }
                key = f"{name}_tok{tok}_{dname}"
                y, yg = routes["gemv"]().float(), routes["gemm"]().float()
                res["check_rel"][key] = float((y - yg).norm() / yg.norm())
                reps = 20
                out = res["calls_us"][key] = {}
                with torch.no_grad():
                    for rnd in (1, 2):
                        for rname, fn in routes.items():
                            for _ in range(10):
                                fn()
                            ts = []
                            for _ in range(args.samples):
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
                med = min(out["gemv_run1"][0], out["gemv_run2"][0])
                bps = p.codes.numel() / (med * 1e-6)
                res["gemv_stream"][key] = {"bytes": int(p.codes.numel()), "bytes_per_s": round(bps, -6),
                                           "hbm_share": round(bps / HBM_BYTES_PER_S, 4)}
                print(key, json.dumps(out), json.dumps(res["gemv_stream"][key]), flush=True)
                json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
