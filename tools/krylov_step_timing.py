#!/usr/bin/env python3
"""Timing of the fused Krylov block step against the default route, on one
MI355X at the notebook's shape (4096 x 4096 float32 X):

  1. orthonormalize(Z) at k = 32 and 64, fused against default;
  2. one re-orthogonalisation pass at p = 32 / 128 / 512 and k = 32 / 64:
     panel.reorth(K, panel.gram(K, Z), Z) against Z - K @ panel.gram(K, Z);
  3. a whole warm-started KrylovProjector call at rank 8 and 64, fused against default.

The two routes alternate in one process after a warm-up; each sample is a host clock around
`inner` calls that end in a device synchronise. Medians and p10 / p90 per cell, and whether
the two p10-p90 ranges are apart. Prints one JSON line; --out also writes it to a file.
usage: tools/krylov_step_timing.py [--reps 30] [--out profiles/krylov_fused_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "admm-quantization_amd")]
import torch  # noqa: E402

from admmq import panel  # noqa: E402
from admmq.lowrank import KrylovProjector, orthonormalize  # noqa: E402


def compare(default, fused, reps, inner, warmup=3):
    """Alternating samples of the two callables: microseconds per call."""
    samples = {"default": [], "fused": []}
    for it in range(warmup + reps):
        for name, fn in (("default", default), ("fused", fused)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            if it >= warmup:
                samples[name].append((time.perf_counter() - t0) / inner * 1e6)
    out = {}
    for name, v in samples.items():
        q = torch.quantile(torch.tensor(v, dtype=torch.float64), torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64))
        out[name] = {"median_us": float(q[1]), "p10_us": float(q[0]), "p90_us": float(q[2])}
    d, f = out["default"], out["fused"]
    out["ranges_apart"] = f["p90_us"] < d["p10_us"] or d["p90_us"] < f["p10_us"]
    out["default_over_fused"] = d["median_us"] / f["median_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("krylov_step_timing needs a ROCm GPU")
    dev = torch.device("cuda:0")
    n = a.size
    g = torch.Generator().manual_seed(0)
    X = torch.randn(n, n, generator=g).to(dev)
    cells = {}
    for k in (32, 64):
        Z = torch.randn(n, k, generator=g, dtype=torch.float64).to(dev)
        cells[f"orthonormalize_k{k}"] = compare(lambda: orthonormalize(Z), lambda: orthonormalize(Z, fused=True), a.reps, 20)
        for p in (32, 128, 512):
            K = torch.linalg.qr(torch.randn(n, p, generator=g, dtype=torch.float64).to(dev))[0]
            cells[f"reorth_pass_p{p}_k{k}"] = compare(lambda: Z - K @ panel.gram(K, Z),
                                                     lambda: panel.reorth(K, panel.gram(K, Z), Z), a.reps, 20)
    for rank in (8, 64):
        pd, pf = KrylovProjector(rank), KrylovProjector(rank, fused=True)
        pd(X), pf(X)   # cold calls: the timed ones start from the previous call's Ritz vectors
        cells[f"projector_rank{rank}"] = compare(lambda: pd(X), lambda: pf(X), a.reps, 1)
        cells[f"projector_rank{rank}"]["blocks"] = {"default": pd.blocks[-1], "fused": pf.blocks[-1]}
        cells[f"projector_rank{rank}"]["repairs"] = {"default": pd.repairs, "fused": pf.repairs}
    out = {"config": f"{n} x {n} float32 X, float64 panels; {a.reps} alternating samples per route after 3 warm-up rounds; "
                     "microseconds per call, host clock around calls ending in a device synchronise",
           "device": torch.cuda.get_device_name(0), "cells": cells}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
