#!/usr/bin/env python3
"""Timing of the skinny quant + low-rank GEMV on the MI355X against the route a user
had before it. Writes profiles/packed_lrgemv_timing.json.

Routes, alternating within one job (two rounds), for float32 and bfloat16 activations at 4 bits
(tensor_mseminmax_symmetric), ranks 8 and 64, 1 / 4 / 8 tokens, on the C5 Llama shapes:
  lrgemv    packed_lowrank_linear(x, p, skinny=True): k_lr_down_gemv + k_packed_lrgemv
  lrgemm    packed_lowrank_linear(x, p): today's route (float32: k_lr_down + k_packed_lrgemm on the
            64 x 64 MFMA tile; bfloat16: the half packed GEMM plus two library products), the yardstick
  gemv      packed_linear(x, p.q, skinny=True): W_q alone - the price of the tail (context only)
  resident  F.linear on a resident dense weight of x's dtype (context only)
`verdict` per cell: "below" when in both rounds lrgemv's median is below lrgemm's and their p10-p90
ranges do not overlap, else "miss" - reported, not re-run.
Method (tools/packed_gemv_timing.py's): HIP events around `reps` back-to-back calls, 10 warm-up calls,
`samples` samples, median [p10, p90] in microseconds per call from Python on one stream.
usage: packed_lrgemv_timing.py --out FILE [--samples 20] [--only SUBSTR]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))

BITS, SCHEME = 4, "tensor_mseminmax_symmetric"
TOKENS = [1, 4, 8]
RANKS = [8, 64]
CASES = [("llama_M4096_K4096", (4096, 4096)), ("llama_M11008_K4096", (11008, 4096)), ("llama_M4096_K11008", (4096, 11008))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from admmq import PackedLowRank, packed_linear, packed_lowrank_linear, quantize_packed
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "check_rel": {}, "verdict": {},
           "method": "median [p10, p90] us per call; two alternating rounds; below: lrgemv under lrgemm, ranges apart, both rounds"}
    for name, shape in CASES:
        if args.only and args.only not in name:
            continue
        M, K = shape
        q = quantize_packed([(torch.randn(M, K, generator=g) * 0.05).to(dev)], BITS, SCHEME)[0]
        D = q.dequantize()
        for r in RANKS:
            p = PackedLowRank(q=q, L=(torch.randn(M, r, generator=g) * 0.05).to(dev), Rt=(torch.randn(r, K, generator=g) * 0.05).to(dev))
            W = D + p.L @ p.Rt
            for dtype, dname in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
                Wres = W.to(dtype)
                for tok in TOKENS:
                    x = torch.randn(tok, K, generator=g).to(dev).to(dtype)
                    routes = {
                        "lrgemv": lambda: packed_lowrank_linear(x, p, skinny=True),
                        "lrgemm": lambda: packed_lowrank_linear(x, p),
                        "gemv": lambda: packed_linear(x, q, skinny=True),
                        "resident": lambda: F.linear(x, Wres),
                    }
                    key = f"{name}_r{r}_tok{tok}_{dname}"
                    y, yg = routes["lrgemv"]().float(), routes["lrgemm"]().float()
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
                    below = all(out[f"lrgemv_run{n}"][0] < out[f"lrgemm_run{n}"][0] and out[f"lrgemv_run{n}"][2] < out[f"lrgemm_run{n}"][1]
                                for n in (1, 2))
                    res["verdict"][key] = "below" if below else "miss"
                    print(key, res["verdict"][key], json.dumps(out), flush=True)
                    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
