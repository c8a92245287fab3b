#!/usr/bin/env python3
"""Timing of the skinny integer GEMV on the MI355X against packed_linear_int's default
route (the int8 MFMA tile route, what a user had before it). Writes profiles/packed_igemv_timing.json.

Routes, alternating within one job (two rounds), for 8-bit activation codes at 1 / 4 / 8 rows and weight
widths 2, 4 and 8 bits:
  igemv  packed_linear_int(xq, p, skinny=True): k_packed_igemv / k_packed_igemv_t (+ k_packed_igemv_reduce)
  igemm  packed_linear_int(xq, p): k_packed_igemm (+ k_packed_ireduce), the yardstick
Cells: the two stages of a CP-FC classifier pair (512 -> R = 256 -> 1000: fc1 is D^T, fc2 is D) and the decode
shapes of tools/packed_gemv_timing.py in both orientations. Per cell the two outputs are compared with
torch.equal, the plan (ks, ns) is recorded, and `ratio` is igemm's median over igemv's (above 1: the skinny
route is faster). The times are per call from Python, back to back on one stream: they hold the call's host
cost, which both routes pay.
Method (tools/packed_gemv_timing.py's): HIP events around `reps` back-to-back calls, 10 warm-up calls,
`samples` samples, median [p10, p90] in microseconds per call. Run it under a time limit of its own:
  timeout -k 10 900 python tools/packed_igemv_timing.py --out profiles/packed_igemv_timing.json
usage: packed_igemv_timing.py --out FILE [--samples 20] [--only SUBSTR]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))

SCHEME = "tensor_mseminmax_symmetric"
BITS = [2, 4, 8]
ROWS = [1, 4, 8]
XBITS, XMN, XRNG = 8, -4.0, 8.0
# (name, packed shape, transpose)
CASES = [
    ("cpfc_fc1_M256_K512_T", (512, 256), True),
    ("cpfc_fc2_M1000_K256", (1000, 256), False),
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
    from admmq import QuantizedActivation, _lib, packed_linear_int, quantize_packed
    from admmq.packed import _meta_words, _weight_dims
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "equal": {}, "plan": {}, "ratio": {},
           "method": "median [p10, p90] us per call; two alternating rounds; ratio: igemm median / igemv median (best round each)"}
    for name, shape, tr in CASES:
        if args.only and args.only not in name:
            continue
        W = (torch.randn(*shape, generator=g) * 0.05).to(dev)
        for bits in BITS:
            p = quantize_packed([W], bits, SCHEME)[0]
            M, K = _weight_dims(p, tr)
            meta, plan = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes()), (ctypes.c_int32 * 3)()
            assert _lib.load().admmq_packed_igemv_plan(ctypes.byref(meta), 1 if tr else 0, M, K, plan) == 0
            for rows in ROWS:
                xc = torch.randint(0, 1 << XBITS, (rows, K), generator=g, dtype=torch.int32).to(torch.uint8).to(dev)
                xq = QuantizedActivation(xc, XBITS, XMN, XRNG)
                routes = {
                    "igemv": lambda: packed_linear_int(xq, p, None, tr, skinny=True),
                    "igemm": lambda: packed_linear_int(xq, p, None, tr),
                }
                key = f"{name}_b{bits}_n{rows}"
                res["equal"][key] = bool(torch.equal(routes["igemv"](), routes["igemm"]()))
                res["plan"][key] = {"ks": plan[0], "ns": plan[1]}
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
                res["ratio"][key] = round(min(out["igemm_run1"][0], out["igemm_run2"][0]) /
                                          min(out["igemv_run1"][0], out["igemv_run2"][0]), 3)
                print(key, json.dumps(out), res["plan"][key], "equal", res["equal"][key], "ratio", res["ratio"][key], flush=True)
                json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
