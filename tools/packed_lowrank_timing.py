#!/usr/bin/env python3
"""Timing of the packed quant + low-rank linear layer on the MI355X: 4 bits,
the Llama shapes of config C5, r in {8, 64}, 1 / 16 / 512 tokens.

Routes, alternating within one process (two rounds):
  fused        packed_lowrank_linear: k_lr_down + k_packed_lrgemm (+ k_lr_reduce)
  composition  packed_linear(x, p.q) + (x @ Rt.T) @ L.T: the packed GEMM, two library GEMMs and an add
  dense        F.linear(x, W_q + W_r) on a resident float32 weight (what the route saved before)
Method: HIP events around `reps` back-to-back calls, 10 warm-up calls, `samples` samples,
median [p10, p90] in microseconds per call; resident weight bytes of each form beside them.
usage: packed_lowrank_timing.py --out FILE [--samples 40]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))

BITS, SCHEME = 4, "tensor_mseminmax_symmetric"
SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008)]
RANKS = [8, 64]
TOKENS = [1, 16, 512]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=40)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from admmq import PackedLowRank, packed_linear, packed_lowrank_linear, quantize_packed
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "check_rel": {}, "resident_bytes": {}}
    for M, K in SHAPES:
        q = quantize_packed([(torch.randn(M, K, generator=g) * 0.02).to(dev)], BITS, SCHEME)[0]
        for r in RANKS:
            p = PackedLowRank(q=q, L=(torch.randn(M, r, generator=g) * 0.1).to(dev),
                              Rt=(torch.randn(r, K, generator=g) * 0.1).to(dev))
            W = p.dequantize()                          # W_q + L Rt, resident float32
            LT, RT = p.L.T, p.Rt.T
            res["resident_bytes"][f"M{M}_K{K}_r{r}"] = {"packed": p.nbytes, "dense_q_plus_r": 8 * M * K, "dense_sum": 4 * M * K}
            for tok in TOKENS:
                x = torch.randn(tok, K, generator=g).to(dev)
                routes = {
                    "fused": lambda: packed_lowrank_linear(x, p),
                    "composition": lambda: packed_linear(x, p.q) + (x @ RT) @ LT,
                    "dense": lambda: F.linear(x, W),
                }
                key = f"M{M}_K{K}_r{r}_tok{tok}"
                y, yc, yd = routes["fused"](), routes["composition"](), routes["dense"]()
                res["check_rel"][key] = {"vs_composition": float((y - yc).norm() / yc.norm()),
                                         "vs_dense": float((y - yd).norm() / yd.norm())}
                reps = 4 if tok > 256 else 20
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
                print(key, json.dumps(out), flush=True)
            del W, p
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
