#!/usr/bin/env python3
"""Timing of the integer quant + low-rank GEMM on the MI355X against the routes a caller holding
activation codes and a PackedLowRank has without it. Writes profiles/packed_ilrgemm_timing.json.

Routes, alternating within one job (two rounds), for 8-bit activation codes, weight bits 4 and 8
(tensor_mseminmax_symmetric), ranks 32 and 128, 16 / 64 / 512 / 2048 rows, on the C5 Llama shapes:
  ilr       packed_lowrank_linear_int(xq, p): k_ilr_down + k_packed_ilrgemm (+ k_packed_ilrreduce), bfloat16 tail
  decode32  act_decode + packed_lowrank_linear on the float32 result: today's only route from codes, the yardstick
  hlr       packed_hlrgemm on a bfloat16 copy of the decoded input (made once, outside the timed region; context:
            another function, the codes are rounded to bfloat16)
  int       packed_linear_int alone (no L Rt): what the tail costs on top of it
The tool asserts that ilr agrees with decode32 within the sum of their bounds (2.37's for ilr,
(K + r + 6) 2^-23 (|D||x| + |L|(|Rt||x|)) for decode32 as in 2.28), evaluated in float64 on the device.
`verdict` per cell: "below" when in both rounds ilr's median is below decode32's and their p10-p90 ranges do not
overlap, else "miss" - reported, not re-run. `best_us`: per route the round with the lower median. `plan`:
(np, parallel, nsd, launches).
Method (tools/packed_hlrgemm_timing.py's): HIP events around `reps` back-to-back calls, 10 warm-up calls,
`samples` samples, median [p10, p90] in microseconds per call from Python on one stream.
usage: packed_ilrgemm_timing.py --out FILE [--samples 20] [--only SUBSTR]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))

SCHEME = "tensor_mseminmax_symmetric"
WBITS = [4, 8]
ROWS = [16, 64, 512, 2048]
RANKS = [32, 128]
XQ = (8, -3.0, 3.0)
CASES = [("llama_M4096_K4096", (4096, 4096)), ("llama_M11008_K4096", (11008, 4096)), ("llama_M4096_K11008", (4096, 11008))]
ULP = 2.0 ** -23


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    from admmq import (PackedLowRank, _lib, act_decode, act_encode, packed_hlrgemm, packed_linear_int, packed_lowrank_linear,
                       packed_lowrank_linear_int, quantize_packed)
    from admmq.packed import _meta_words
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "best_us": {}, "check_err_over_bound": {}, "plan": {}, "verdict": {},
           "method": "median [p10, p90] us per call; two alternating rounds; best_us: the round with the lower median; "
                     "below: ilr under decode32, ranges apart, both rounds"}
    T, u = torch.bfloat16, 2.0 ** -8
    for name, (M, K) in CASES:
        if args.only and args.only not in name:
            continue
        W = (torch.randn(M, K, generator=g) * 0.05).to(dev)
        for wb in WBITS:
            q = quantize_packed([W], wb, SCHEME)[0]
            D = q.dequantize()
            for r in RANKS:
                L32, R32 = (torch.randn(M, r, generator=g) * 0.05).to(dev), (torch.randn(r, K, generator=g) * 0.05).to(dev)
                p = PackedLowRank(q=q, L=L32.to(T).float(), Rt=R32.to(T).float())
                for rows in ROWS:
                    xq = act_encode(torch.randn(rows, K, generator=g).to(dev), XQ, check=False)
                    xh = act_decode(xq.codes, xq.bits, xq.mn, xq.rng).to(T)
                    routes = {
                        "ilr": lambda: packed_lowrank_linear_int(xq, p),
                        "decode32": lambda: packed_lowrank_linear(act_decode(xq.codes, xq.bits, xq.mn, xq.rng), p),
                        "hlr": lambda: packed_hlrgemm(q.codes, _meta_words(q), M, K, p.L, p.Rt, xh, None, torch.float32),
                        "int": lambda: packed_linear_int(xq, q),
                    }
                    key = f"{name}_w{wb}_r{r}_rows{rows}"
                    out4 = (ctypes.c_int32 * 4)()
                    assert lib.admmq_packed_ilrgemm_plan(M, K, rows, r, out4) == 0
                    res["plan"][key] = list(out4)
                    ya, yb = routes["ilr"]().double(), routes["decode32"]().double()
                    X = act_decode(xq.codes, xq.bits, xq.mn, xq.rng).double().abs()   # <= g ux + |mn_x| elementwise
                    A, B = X @ D.double().abs().T, (X @ p.Rt.double().abs().T) @ p.L.double().abs().T
                    gm, gd = (1.0 + ULP) ** (K + r + 4) - 1.0, (K + r + 6) * ULP
                    Bx = ((X + abs(xq.mn)) @ p.Rt.double().abs().T) @ p.L.double().abs().T
                    bound = gm * Bx + u * (1 + gm) * Bx + ULP * ya.abs() + gd * (A + B)
                    res["check_err_over_bound"][key] = float(((ya - yb).abs() / bound.clamp_min(1e-300)).max())
                    assert res["check_err_over_bound"][key] <= 1.0, (key, res["check_err_over_bound"][key])
                    del ya, yb, X, A, B, Bx, bound
                    reps = 5 if rows >= 512 else 20
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
                    res["best_us"][key] = {rn: min(out[f"{rn}_run1"], out[f"{rn}_run2"]) for rn in routes}
                    below = all(out[f"ilr_run{n}"][0] < out[f"decode32_run{n}"][0] and out[f"ilr_run{n}"][2] < out[f"decode32_run{n}"][1]
                                for n in (1, 2))
                    res["verdict"][key] = "below" if below else "miss"
                    print(key, res["verdict"][key], res["plan"][key], json.dumps(res["best_us"][key]), flush=True)
                    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
