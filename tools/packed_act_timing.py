#!/usr/bin/env python3
"""Timing of the fixed-range activation quantizers fused into the packed kernels
against the routes they replace, on the MI355X. Writes profiles/packed_act_timing.json's
"calls_us" part.

Cases: the three fused depthwise + 1x1 cases of packed_cp_timing.py and packed_conv1x1 at
layer2 M128 K286 28x28 nb 64. Routes, alternating within one job (two rounds), all with the same
8 bit output quantizer ("same_bits" records whether a route's result equals the fused one; the torch
ops of `eager` need not round as the reference's CPU code does):
  fused       the quantizer in the kernel's epilogue (act=)
  two_launch  the packed call, then k_fixed_quant (min_max_quantize) on its result
  eager       the packed call, then the reference's formula as torch ops (what the library
              offered before the quantizers: the baseline)
  plain       the packed call alone (the floor; fused - plain is the epilogue's cost)
  fused_mid   (fused stage only) the mid quantizer in the kernel as well: reported, not compared
Method: HIP events around `reps` back-to-back calls, 10 warm-up calls, `samples` samples,
median [p10, p90] in microseconds per call. "requirements": per case, the fused median (mean of
the two rounds) lies below the eager one by more than the largest spread between a route's two
rounds; in the activation-bound cases (nb 64) the same against two_launch.
  --trace   few calls per route, for a `rocprofv3 --kernel-trace --stats` run of its own
  --kernels DIR   read that run's kernel_trace.csv and add "kernels_us" to the JSON
usage: packed_act_timing.py --out FILE [--samples 40] [--trace] [--kernels DIR]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BITS, SCHEME = 4, "tensor_mseminmax_symmetric"
ABITS = 8
# (name, M, R, (H, W), k (0: packed_conv1x1), pad, stride, nb)
CASES = [
    ("layer4_tail_M512_R1141_7x7_nb1", 512, 1141, (7, 7), 3, 1, 1, 1),
    ("layer4_tail_M512_R1141_7x7_nb64", 512, 1141, (7, 7), 3, 1, 1, 64),
    ("layer2_down_M128_R286_56x56_s2_nb1", 128, 286, (56, 56), 3, 1, 2, 1),
    ("layer2_conv1x1_M128_K286_28x28_nb64", 128, 286, (28, 28), 0, 0, 1, 64),
]
ACTIVATION_BOUND = [c[0] for c in CASES if c[7] == 64]


def main():
    from packed_gemm_timing import kernels
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
    from admmq import min_max_quantize, packed_conv1x1, packed_depthwise_conv1x1, quantize_packed
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "same_bits": {}, "requirements": {}}

    def eager_q(y, mn, rng, n):   # the reference's formula, one torch launch per step
        return torch.floor((y - mn) / rng * n + 0.5) * rng / n + mn

    for name, M, R, (H, W), k, pad, stride, nb in CASES:
        A = quantize_packed([(torch.randn(M, R, generator=g) * 0.05).to(dev)], BITS, SCHEME)[0]
        bias = torch.randn(M, generator=g).to(dev)
        t = torch.randn(nb, R, H, W, generator=g).to(dev)
        if k:
            taps = quantize_packed([(torch.randn(k * k, R, generator=g) * 0.3).to(dev)], BITS, SCHEME)[0].dequantize()
            call = lambda **q: packed_depthwise_conv1x1(t, taps, A, bias, (k, k), stride, pad, **q)   # noqa: E731
        else:
            call = lambda **q: packed_conv1x1(t, A, bias, **q)   # noqa: E731
        with torch.no_grad():
            y0 = call()
            lo, hi = torch.quantile(y0.reshape(-1)[:1 << 20].float(), torch.tensor([0.02, 0.98], device=dev)).tolist()
            act = (ABITS, lo, hi)
            # (two Python numbers: the range is their double difference rounded once)
            mn_t, rng_t, n_t = torch.tensor(lo, device=dev), torch.tensor(hi - lo, device=dev), float(2 ** ABITS - 1)
            routes = {
                "fused": lambda: call(act=act),
                "two_launch": lambda: min_max_quantize(call(), *act),
                "eager": lambda: eager_q(call(), mn_t, rng_t, n_t),
                "plain": call,
            }
            if k:
                routes["fused_mid"] = lambda: call(act=act, mid_act=(ABITS, -2.0, 2.0))
            yf = routes["fused"]()
            res["same_bits"][name] = {"two_launch": bool(torch.equal(yf, routes["two_launch"]())),
                                      "eager": bool(torch.equal(yf, routes["eager"]()))}
            cols = y0.numel() // M
            reps = 4 if cols > 256 else 20
            nsamp = 3 if args.trace else args.samples
            out = res["calls_us"][name] = {}
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
        print(name, json.dumps(out), flush=True)
        med = {r: sorted(out[f"{r}_run{n}"][0] for n in (1, 2)) for r in ("fused", "two_launch", "eager", "plain")}
        mean = {r: round(sum(v) / 2, 1) for r, v in med.items()}
        spread = round(max(v[1] - v[0] for v in med.values()), 1)
        req = dict(mean, round_spread_us=spread, epilogue_cost_us=round(mean["fused"] - mean["plain"], 1),
                   fused_below_eager=bool(mean["fused"] + spread < mean["eager"]))
        if name in ACTIVATION_BOUND:
            req["fused_below_two_launch"] = bool(mean["fused"] + spread < mean["two_launch"])
        res["requirements"][name] = req
        print("requirement", name, json.dumps(req), flush=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
