#!/usr/bin/env python3
"""Timing of the integer packed GEMM against the float packed GEMM and the
library on a resident float32 weight, on the MI355X, on the seven shapes of DESIGN.md 2.22's
table. Writes profiles/packed_igemm_timing.json.

Routes, alternating within one job (two rounds):
  integer   packed_conv1x1_int / packed_linear_int: codes in (encoded before the timed region),
            float out; the weight's row sums are on the packed tensor before the first sample
  fused     packed_conv1x1 / packed_linear on the float input (k_packed_gemm)
  resident  F.conv2d / F.linear on an already resident float32 weight
Also: k_act_encode on a 64 x 286 x 28 x 28 tensor, k_packed_rowsum on the three weights (both as
"extra_us"), and the 2-way integer layer against the float packed layer with the same quantizers
at (4096, 1024), R = 24, for 16 and 512 tokens ("layers_us").
Method: HIP events around `reps` back-to-back calls, 10 warm-up calls, `samples` samples,
median [p10, p90] in microseconds per call. "goals" compares the integer and the fused medians of
each shape (a route's median: the mean of its two rounds' medians) with the shape's round spread
(the largest difference between the two rounds of one of its routes).
  --trace   few calls per route, for a `rocprofv3 --kernel-trace` run of its own
  --kernels DIR   read that run's kernel_trace.csv and add "kernels_us" to the JSON
usage: packed_igemm_timing.py --out FILE [--samples 40] [--trace] [--kernels DIR]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from packed_gemm_timing import BITS, CASES, SCHEME, kernels   # noqa: E402  (the same shapes and trace reader)

XACT = (8, -4.0, 4.0)
LARGE = ("N3136", "tok512")


def timed(fn, reps, nsamp):
    import torch
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
    return [round(ts[len(ts) // 2], 1), round(ts[len(ts) // 10], 1), round(ts[(9 * len(ts)) // 10], 1)]


def rounds(routes, reps, nsamp):
    out = {}
    for rnd in (1, 2):
        for rname, fn in routes.items():
            out[f"{rname}_run{rnd}"] = timed(fn, reps, nsamp)
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
    from admmq import (act_encode, export, packed_conv1x1, packed_conv1x1_int, packed_linear, packed_linear_int,
                       packed_rowsums, quantize_packed)
    from admmq.packed import _meta_words, _rowsums, _weight_dims
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    nsamp = 3 if args.trace else args.samples
    res = {"calls_us": {}, "check_rel": {}, "goals": {}, "extra_us": {}, "layers_us": {}}
    with torch.no_grad():
        for name, kind, shape, tr, acts in CASES:
            p = quantize_packed([(torch.randn(*shape, generator=g) * 0.05).to(dev)], BITS, SCHEME)[0]
            D = p.dequantize()
            Wres = (D.T if tr else D).contiguous()
            M, K = Wres.shape
            packed_rowsums(p, tr)
            res["extra_us"][f"rowsum_{name}"] = timed(lambda: _rowsums(p.codes, _meta_words(p), tr, *_weight_dims(p, tr)),
                                                      20, nsamp)
            for label, xs in acts:
                x = torch.randn(*xs, generator=g).clamp_(-3.9, 3.9).to(dev)
                xq = act_encode(x, XACT)
                C = x.numel() // K
                if kind == "conv":
                    routes = {
                        "integer": lambda: packed_conv1x1_int(xq, p, transpose=tr),
                        "fused": lambda: packed_conv1x1(x, p, transpose=tr),
                        "resident": lambda: F.conv2d(x, Wres[:, :, None, None]),
                    }
                else:
                    routes = {
                        "integer": lambda: packed_linear_int(xq, p, transpose=tr),
                        "fused": lambda: packed_linear(x, p, transpose=tr),
                        "resident": lambda: F.linear(x, Wres),
                    }
                key = f"{name}_{label}"
                y, yr = routes["integer"](), routes["resident"]()
                res["check_rel"][key] = float((y - yr).norm() / yr.norm())   # (the input's 8-bit quantization)
                out = res["calls_us"][key] = rounds(routes, 4 if C > 256 else 20, nsamp)
                spread = max(abs(out[f"{r}_run1"][0] - out[f"{r}_run2"][0]) for r in routes)
                ig, fu = [out[f"integer_run{r}"][0] for r in (1, 2)], [out[f"fused_run{r}"][0] for r in (1, 2)]
                mi, mf = sum(ig) / 2, sum(fu) / 2   # a route's median: the mean of its two rounds' medians
                large = label in LARGE
                res["goals"][key] = {
                    "kind": "below fused by more than the spread" if large else "not above fused by more than the spread",
                    "integer": round(mi, 2), "fused": round(mf, 2), "round_spread": round(spread, 1),
                    "met": bool(mi < mf - spread if large else mi <= mf + spread),
                    # the stricter reading: the integer route's worse round against the fused route's better one
                    "met_worst_round": bool(max(ig) < min(fu) - spread if large else max(ig) <= min(fu) + spread)}
                print(key, json.dumps(out), json.dumps(res["goals"][key]), flush=True)
        x = torch.randn(64, 286, 28, 28, generator=g).clamp_(-3.9, 3.9).to(dev)
        res["extra_us"]["act_encode_64x286x28x28"] = timed(lambda: act_encode(x, XACT, check=False), 4, nsamp)
        del x
        fout, fin, R = 4096, 1024, 24
        pf = quantize_packed([(torch.randn(fout, R, generator=g) * 0.05).to(dev),
                              (torch.randn(fin, R, generator=g) * 0.05).to(dev)], BITS, SCHEME)
        for tok in (16, 512):
            x = torch.randn(tok, fin, generator=g).clamp_(-3.9, 3.9).to(dev)
            plain = export.build_cpfc_layer(R, pf, None, fin, fout)
            h = plain.fc1(x)
            acts = [(8, float(h.min()) - 0.05, float(h.max()) + 0.05), None]
            fl = export.build_cpfc_layer(R, pf, None, fin, fout, act_quant=acts)
            il = export.build_cpfc_layer(R, pf, None, fin, fout, act_quant=acts, integer=True, in_act=XACT)
            res["layers_us"][f"cpfc_4096x1024_R24_tok{tok}"] = rounds({"integer": lambda: il(x), "fused": lambda: fl(x)},
                                                                       20, nsamp)
            print(tok, json.dumps(res["layers_us"][f"cpfc_4096x1024_R24_tok{tok}"]), flush=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
