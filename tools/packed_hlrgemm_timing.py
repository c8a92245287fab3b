#!/usr/bin/env python3
"""Timing of the half-precision fused quant + low-rank GEMM on the MI355X against the
route a user has without the flag. Writes profiles/packed_hlrgemm_timing.json.

Routes, alternating within one job (two rounds), for bfloat16 and float16 activations at 4 bits
(tensor_mseminmax_symmetric), ranks 8 and 64, 16 / 64 / 512 tokens, on the C5 Llama shapes:
  fused     packed_lowrank_linear(x, p, fused=True): k_hlr_down + k_packed_hlrgemm (+ k_packed_hlrreduce)
  default   packed_lowrank_linear(x, p): today's route, untouched (the half packed GEMM with a float32
            result, x.float(), two library products, the elementwise passes), the yardstick
  f32       packed_lowrank_linear(x.float(), p): the fused float32 kernels of 2.28 (context only)
  resident  F.linear on a resident dense weight of x's dtype (context only)
The factors are rounded to x's dtype first, so both routes evaluate the same function; the tool asserts
that they agree within the sum of their bounds (2.35's for fused, (K + r + 6) 2^-23 (|D||x| + |L|(|Rt||x|))
for default as in 2.33), evaluated in float64 on the device.
`verdict` per cell: "below" when in both rounds fused's median is below default's and their p10-p90
ranges do not overlap, else "miss" - reported, not re-run. `plan`: (np, parallel, nsd, launches).
Method (tools/packed_lrgemv_timing.py's): HIP events around `reps` back-to-back calls, 10 warm-up calls,
`samples` samples, median [p10, p90] in microseconds per call from Python on one stream.
usage: packed_hlrgemm_timing.py --out FILE [--samples 20] [--only SUBSTR]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))

BITS, SCHEME = 4, "tensor_mseminmax_symmetric"
TOKENS = [16, 64, 512]
RANKS = [8, 64]
CASES = [("llama_M4096_K4096", (4096, 4096)), ("llama_M11008_K4096", (11008, 4096)), ("llama_M4096_K11008", (4096, 11008))]
ULP = 2.0 ** -23


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from admmq import PackedLowRank, _lib, packed_lowrank_linear, quantize_packed
    from admmq.packed import _meta_words
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "check_err_over_bound": {}, "plan": {}, "verdict": {},
           "method": "median [p10, p90] us per call; two alternating rounds; below: fused under default, ranges apart, both rounds"}
    for name, shape in CASES:
        if args.only and args.only not in name:
            continue
        M, K = shape
        q = quantize_packed([(torch.randn(M, K, generator=g) * 0.05).to(dev)], BITS, SCHEME)[0]
        meta = _lib.QMeta.from_buffer_copy(_meta_words(q).numpy().tobytes())
        D = q.dequantize()
        for r in RANKS:
            L32, R32 = (torch.randn(M, r, generator=g) * 0.05).to(dev), (torch.randn(r, K, generator=g) * 0.05).to(dev)
            for dtype, dname, u in ((torch.bfloat16, "bf16", 2.0 ** -8), (torch.float16, "f16", 2.0 ** -11)):
                p = PackedLowRank(q=q, L=L32.to(dtype).float(), Rt=R32.to(dtype).float())
                Wres = (D + p.L @ p.Rt).to(dtype)
                for tok in TOKENS:
                    x = torch.randn(tok, K, generator=g).to(dev).to(dtype)
                    xf = x.float()
                    routes = {
                        "fused": lambda: packed_lowrank_linear(x, p, fused=True),
                        "default": lambda: packed_lowrank_linear(x, p),
                        "f32": lambda: packed_lowrank_linear(xf, p),
                        "resident": lambda: F.linear(x, Wres),
                    }
                    key = f"{name}_r{r}_tok{tok}_{dname}"
                    out4 = (ctypes.c_int32 * 4)()
                    assert lib.admmq_packed_hlrgemm_plan(ctypes.byref(meta), M, K, tok, r, out4) == 0
                    res["plan"][key] = list(out4)
                    ya = packed_lowrank_linear(x, p, out_dtype=torch.float32, fused=True).double()
                    yb = packed_lowrank_linear(x, p, out_dtype=torch.float32).double()
                    X = x.double().abs()
                    A, B = X @ D.double().abs().T, (X @ p.Rt.double().abs().T) @ p.L.double().abs().T
                    gm = (1.0 + ULP) ** (K + r + 6) - 1.0
                    bound = gm * (A + B) + u * (1 + gm) * B + 2.0 ** -25 * (1 + gm) * p.L.double().abs().sum(1) + (K + r + 6) * ULP * (A + B)
                    res["check_err_over_bound"][key] = float(((ya - yb).abs() / bound.clamp_min(1e-300)).max())
                    assert res["check_err_over_bound"][key] <= 1.0, (key, res["check_err_over_bound"][key])
                    del ya, yb, X, A, B, bound
                    reps = 5 if tok >= 512 else 20
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
                    below = all(out[f"fused_run{n}"][0] < out[f"default_run{n}"][0] and out[f"fused_run{n}"][2] < out[f"default_run{n}"][1]
                                for n in (1, 2))
                    res["verdict"][key] = "below" if below else "miss"
                    print(key, res["verdict"][key], res["plan"][key], json.dumps(out), flush=True)
                    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
