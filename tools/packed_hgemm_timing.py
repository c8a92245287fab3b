#!/usr/bin/env python3
"""Timing of the half-precision packed GEMM on the MI355X against the route a user
had before it and against a dense half weight. Writes profiles/packed_hgemm_timing.json.

Routes, alternating within one job (two rounds), for bfloat16 and float16 activations at 4 bits:
  half      packed_conv1x1 / packed_linear on the half x: one call on the 16-bit MFMA
  cast      packed_*(x.float(), p).to(dtype): the float32 kernel between two conversion passes,
            all three timed together
  resident  F.conv2d / F.linear on a resident dense weight of x's dtype (context only)
Cases: those of tools/packed_gemm_timing.py and the three Llama shapes of DESIGN.md 2.28 at
1 / 16 / 512 tokens.
Method (tools/packed_gemm_timing.py's): HIP events around `reps` back-to-back calls, 10 warm-up
calls, `samples` samples, median [p10, p90] in microseconds per call.
usage: packed_hgemm_timing.py --out FILE [--samples 30] [--only SUBSTR]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))

BITS, SCHEME = 4, "tensor_mseminmax_symmetric"
TOKENS = [("tok1", 1), ("tok16", 16), ("tok512", 512)]
# (name, kind, packed shape, transpose, [(label, activations shape)])
CASES = [
    ("layer4_conv1_M1141_K512_T", "conv", (512, 1141), True, [("N49", (1, 512, 7, 7)), ("N3136", (64, 512, 7, 7))]),
    ("layer4_conv3_M512_K1141", "conv", (512, 1141), False, [("N49", (1, 1141, 7, 7)), ("N3136", (64, 1141, 7, 7))]),
    ("c5_linear_M4096_K1024", "linear", (4096, 1024), False, [(l, (t, 1024)) for l, t in TOKENS]),
    ("llama_M4096_K4096", "linear", (4096, 4096), False, [(l, (t, 4096)) for l, t in TOKENS]),
    ("llama_M11008_K4096", "linear", (11008, 4096), False, [(l, (t, 4096)) for l, t in TOKENS]),
    ("llama_M4096_K11008", "linear", (4096, 11008), False, [(l, (t, 11008)) for l, t in TOKENS]),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from admmq import packed_conv1x1, packed_linear, quantize_packed
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "check_rel": {}, "method": "median [p10, p90] us per call; two alternating rounds"}
    for name, kind, shape, tr, acts in CASES:
        if args.only and args.only not in name:
            continue
        p = quantize_packed([(torch.randn(*shape, generator=g) * 0.05).to(dev)], BITS, SCHEME)[0]
        D = p.dequantize()
        K = (D.T if tr else D).shape[1]
        for dtype, dname in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
            Wres = (D.T if tr else D).contiguous().to(dtype)
            for label, xs in acts:
                x = torch.randn(*xs, generator=g).to(dev).to(dtype)
                C = x.numel() // K
                if kind == "conv":
                    routes = {
                        "half": lambda: packed_conv1x1(x, p, transpose=tr),
                        "cast": lambda: packed_conv1x1(x.float(), p, transpose=tr).to(dtype),
                        "resident": lambda: F.conv2d(x, Wres[:, :, None, None]),
                    }
                else:
                    routes = {
                        "half": lambda: packed_linear(x, p, transpose=tr),
                        "cast": lambda: packed_linear(x.float(), p, transpose=tr).to(dtype),
                        "resident": lambda: F.linear(x, Wres),
                    }
                key = f"{name}_{label}_{dname}"
                y, yc = routes["half"]().float(), routes["cast"]().float()
                res["check_rel"][key] = float((y - yc).norm() / yc.norm())
                reps = 4 if C > 256 else 20
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
                json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
