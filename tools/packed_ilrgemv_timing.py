#!/usr/bin/env python3
"""Timing of the skinny integer quant + low-rank GEMV on the MI355X against
packed_lowrank_linear_int's default route (the int8 / 16-bit MFMA tile route of 2.37, what a user had before it).
Writes profiles/packed_ilrgemv_timing.json.

Routes, alternating within one job (two rounds), for 8-bit activation codes at 1 / 4 / 8 rows, weight widths 4 and 8
bits, ranks 32 and 128 and a bfloat16 tail:
  ilrgemv  packed_lowrank_linear_int(xq, p, skinny=True): k_ilr_down_gemv + k_packed_ilrgemv (+ k_packed_ilrgemv_reduce)
  ilrgemm  packed_lowrank_linear_int(xq, p): k_ilr_down + k_packed_ilrgemm (+ k_packed_ilrreduce), the yardstick
  igemv    packed_linear_int(xq, p.q, skinny=True) alone, for information: what the tail costs on top
  decode   act_decode + packed_lowrank_linear(skinny=True), for information: the other decode route from codes
Per cell the plan (ks, ns, nsd) is recorded, `ratio` is ilrgemm's median over ilrgemv's (above 1: the skinny route is
faster), `apart` says whether the two p10-p90 ranges of the better rounds do not overlap, and `check` is the largest
|y_ilrgemv - y_ilrgemm| over the sum of the two routes' derived bounds (2.37's and 2.38's, |y64| replaced by the
routes' own |y|); the tool fails above 1. The times are per call from Python, back to back on one stream: they hold
the call's host cost, which every route pays.
Method (tools/packed_igemv_timing.py's): HIP events around `reps` back-to-back calls, 10 warm-up calls, `samples`
samples, median [p10, p90] in microseconds per call. Run it under a time limit of its own:
  timeout -k 10 900 python tools/packed_ilrgemv_timing.py --out profiles/packed_ilrgemv_timing.json
usage: packed_ilrgemv_timing.py --out FILE [--samples 20] [--only SUBSTR]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))

SCHEME = "tensor_mseminmax_symmetric"
BITS = [4, 8]
RANKS = [32, 128]
ROWS = [1, 4, 8]
XBITS, XMN, XRNG = 8, -4.0, 8.0
CASES = [("llama_M4096_K4096", (4096, 4096)), ("llama_M11008_K4096", (11008, 4096)), ("llama_M4096_K11008", (4096, 11008))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    from admmq import (PackedLowRank, QuantizedActivation, _lib, act_decode, packed_linear_int, packed_lowrank_linear,
                       packed_lowrank_linear_int, quantize_packed)
    from admmq.packed import _meta_words
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, T = torch.device("cuda:0"), torch.bfloat16
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "plan": {}, "ratio": {}, "apart": {}, "check": {},
           "method": "median [p10, p90] us per call; two alternating rounds; ratio: ilrgemm median / ilrgemv median (best round each)"}
    eps, u = 2.0 ** -24, 2.0 ** -8
    for name, (M, K) in CASES:
        if args.only and args.only not in name:
            continue
        W = (torch.randn(M, K, generator=g) * 0.05).to(dev)
        for bits in BITS:
            q = quantize_packed([W], bits, SCHEME)[0]
            meta = _lib.QMeta.from_buffer_copy(_meta_words(q).numpy().tobytes())
            for r in RANKS:
                p = PackedLowRank(q=q, L=(torch.randn(M, r, generator=g) * 0.05).to(dev), Rt=(torch.randn(r, K, generator=g) * 0.05).to(dev))
                plan = (ctypes.c_int32 * 4)()
                assert _lib.load().admmq_packed_ilrgemv_plan(ctypes.byref(meta), M, K, r, plan) == 0
                LT, RT = p.L.to(T).double().abs(), p.Rt.to(T).double().abs()
                for rows in ROWS:
                    xc = torch.randint(0, 1 << XBITS, (rows, K), generator=g, dtype=torch.int32).to(torch.uint8).to(dev)
                    xq = QuantizedActivation(xc, XBITS, XMN, XRNG)
                    routes = {
                        "ilrgemv": lambda: packed_lowrank_linear_int(xq, p, tail_dtype=T, skinny=True),
                        "ilrgemm": lambda: packed_lowrank_linear_int(xq, p, tail_dtype=T),
                        "igemv": lambda: packed_linear_int(xq, q, skinny=True),
                        "decode": lambda: packed_lowrank_linear(act_decode(xc, XBITS, XMN, XRNG), p, skinny=True),
                    }
                    key = f"{name}_b{bits}_r{r}_n{rows}"
                    ys, yd = routes["ilrgemv"]().double(), routes["ilrgemm"]().double()
                    B = ((xc.double() * (XRNG / 255) + abs(XMN)) @ RT.T) @ LT.T
                    gs, gd = (1 + eps) ** (K + r + 15) - 1, (1 + 2 * eps) ** (K + r + 4) - 1
                    bound = gs * B + eps * ys.abs() + gd * B + u * (1 + gd) * B + 2 * eps * yd.abs()
                    res["check"][key] = round(float(((ys - yd).abs() / bound).max()), 4)
                    assert res["check"][key] <= 1.0, (key, res["check"][key])
                    res["plan"][key] = {"ks": plan[0], "ns": plan[1], "nsd": plan[2]}
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
                    best = {n: min(out[f"{n}_run1"], out[f"{n}_run2"]) for n in routes}
                    res["ratio"][key] = round(best["ilrgemm"][0] / best["ilrgemv"][0], 3)
                    res["apart"][key] = bool(best["ilrgemv"][2] < best["ilrgemm"][1])
                    print(key, json.dumps(out), res["plan"][key], "check", res["check"][key], "ratio", res["ratio"][key],
                          "apart", res["apart"][key], flush=True)
                    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
