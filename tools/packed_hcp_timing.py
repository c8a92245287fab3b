#!/usr/bin/env python3
"""Timing of the half-precision fused depthwise + 1x1 stage on the MI355X against the
routes a half model has without it. Writes profiles/packed_hdwgemm_timing.json.

Routes, alternating within one job (two rounds), for bfloat16 and float16 activations at 4 bits:
  fused       packed_depthwise_conv1x1 on the half x: one call of k_packed_hdwgemm
  fused_rt1   the same call with ADMMQ_HDW_RT=1: the 64-row tile in the serial regime too (the work-split decision;
              in the parallel regime it is the same kernel)
  cast        packed_depthwise_conv1x1(x.float(), ...).to(dtype): the float32 kernel between two conversion
              passes, all three timed together
  unfused     nn.Conv2d depthwise in the half type + PackedConv1x1 on the half x
Method (tools/packed_hgemm_timing.py's): HIP events around `reps` back-to-back calls, 10 warm-up calls,
`samples` samples, median [p10, p90] in microseconds per call. Kernel times come from a
`--kernel-trace --stats` run of this script of its own (--only, --samples 3).
usage: packed_hcp_timing.py --out FILE [--samples 30] [--only SUBSTR]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))

BITS, SCHEME = 4, "tensor_mseminmax_symmetric"
# (name, M, R, (H, W), stride, nb): 3x3 windows, padding 1
CASES = [
    ("layer4_tail_nb1", 512, 1141, (7, 7), 1, 1),
    ("layer2_down_nb1", 128, 286, (56, 56), 2, 1),
    ("layer4_tail_nb64", 512, 1141, (7, 7), 1, 64),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    from torch import nn
    from admmq import packed_conv1x1, packed_depthwise_conv1x1, quantize_packed
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "check_rel": {}, "method": "median [p10, p90] us per call; two alternating rounds"}
    for name, M, R, (H, W), stride, nb in CASES:
        if args.only and args.only not in name:
            continue
        p = quantize_packed([(torch.randn(M, R, generator=g) * 0.05).to(dev)], BITS, SCHEME)[0]
        taps = (torch.randn(9, R, generator=g) * 0.3).to(dev)
        for dtype, dname in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
            x = torch.randn(nb, R, H, W, generator=g).to(dev).to(dtype)
            dw = nn.Conv2d(R, R, 3, stride=stride, padding=1, groups=R, bias=False).to(dev).to(dtype)
            dw.weight.data.copy_(taps.T.reshape(R, 1, 3, 3))
            kw = dict(kernel_size=3, stride=stride, padding=1)

            def fused_rt1():
                os.environ["ADMMQ_HDW_RT"] = "1"
                try:
                    return packed_depthwise_conv1x1(x, taps, p, **kw)
                finally:
                    del os.environ["ADMMQ_HDW_RT"]

            routes = {
                "fused": lambda: packed_depthwise_conv1x1(x, taps, p, **kw),
                "fused_rt1": fused_rt1,
                "cast": lambda: packed_depthwise_conv1x1(x.float(), taps, p, **kw).to(dtype),
                "unfused": lambda: packed_conv1x1(dw(x), p),
            }
            key = f"{name}_{dname}"
            with torch.no_grad():
                y, y1, yc = routes["fused"](), routes["fused_rt1"](), routes["cast"]().float()
                assert torch.equal(y, y1), "the two work splits must give the same bits"
                res["check_rel"][key] = float((y.float() - yc).norm() / yc.norm())
                reps = 4 if nb > 1 else 20
                out = res["calls_us"][key] = {}
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
