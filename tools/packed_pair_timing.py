#!/usr/bin/env python3
"""Timing of the fused 2-way packed layer against the two-module layer it replaces, on the MI355X.
Writes profiles/packed_pair_timing.json.

Routes, alternating within one job (two rounds), on the same tensors and the same packed factors:
  fused     build_cp2conv_layer / build_cpfc_layer(..., fused=True): one PackedPair, one kernel
  two       the default layer: two PackedConv1x1 / PackedLinear modules, the rank-R tensor through memory
Shapes: resnet50's 2-way 1x1 layers (cout, cin, positions, rank) at batch 1, 8 and 32, and one cpfc head.
Method: HIP events around `reps` back-to-back calls, 10 warm-up calls, `samples` samples, median [p10, p90] in
microseconds per call. "verdict": per case "faster" / "slower" when the two rounds' [p10, p90] ranges of one route lie
wholly on one side of the other route's, else "ranges touch". "plan": (ntile, ms, LDS bytes, workgroups).
usage: packed_pair_timing.py --out FILE [--samples 30]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "admm-quantization_amd"))

BITS, SCHEME = 4, "tensor_mseminmax_symmetric"
# (name, cout, cin, (H, W) or None for cpfc, rank)
LAYERS = [("layer1_64_64_56x56_R16", 64, 64, (56, 56), 16), ("layer1_256_64_56x56_R25", 256, 64, (56, 56), 25),
          ("layer3_1024_256_14x14_R102", 1024, 256, (14, 14), 102), ("layer4_2048_512_7x7_R204", 2048, 512, (7, 7), 204),
          ("cpfc_1000_2048_R128", 1000, 2048, None, 128)]
BATCHES = [1, 8, 32]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=30)
    args = ap.parse_args()
    import torch
    from admmq import quantize_packed
    from admmq.export import build_cp2conv_layer, build_cpfc_layer
    from admmq.packed import packed_pairgemm_plan
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"calls_us": {}, "plan": {}, "check_rel": {}, "verdict": {}}
    for lname, M, K, hw, R in LAYERS:
        A, B = quantize_packed([(torch.randn(M, R, generator=g) * 0.05).to(dev), (torch.randn(K, R, generator=g) * 0.05).to(dev)],
                               BITS, SCHEME)
        bias = torch.randn(M, generator=g).to(dev)
        if hw:
            routes_of = lambda f: build_cp2conv_layer(R, [A, B], bias, K, M, 0, 1, fused=f)
        else:
            routes_of = lambda f: build_cpfc_layer(R, [A, B], bias, K, M, fused=f)
        layers = {"fused": routes_of(True), "two": routes_of(False)}
        for nb in BATCHES:
            name = f"{lname}_nb{nb}"
            x = torch.randn((nb, K) + hw if hw else (nb, K), generator=g).to(dev)
            cols = nb * hw[0] * hw[1] if hw else nb
            res["plan"][name] = list(packed_pairgemm_plan(M, K, cols if not hw else hw[0] * hw[1], nb if hw else 1, R))
            with torch.no_grad():
                y, y2 = layers["fused"](x), layers["two"](x)
                res["check_rel"][name] = float((y - y2).norm() / y2.norm())
                reps = 4 if cols > 4096 else 20
                out = res["calls_us"][name] = {}
                for rnd in (1, 2):
                    for rname, layer in layers.items():
                        for _ in range(10):
                            layer(x)
                        ts = []
                        for _ in range(args.samples):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(reps):
                                layer(x)
                            e1.record()
                            e1.synchronize()
                            ts.append(e0.elapsed_time(e1) * 1e3 / reps)
                        ts.sort()
                        out[f"{rname}_run{rnd}"] = [round(ts[len(ts) // 2], 1), round(ts[len(ts) // 10], 1),
                                                    round(ts[(9 * len(ts)) // 10], 1)]
            lo = {r: min(out[f"{r}_run{n}"][1] for n in (1, 2)) for r in layers}
            hi = {r: max(out[f"{r}_run{n}"][2] for n in (1, 2)) for r in layers}
            res["verdict"][name] = "faster" if hi["fused"] < lo["two"] else ("slower" if lo["fused"] > hi["two"] else "ranges touch")
            print(name, res["plan"][name], json.dumps(out), res["verdict"][name], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
