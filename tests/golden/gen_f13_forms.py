#!/usr/bin/env python3
"""F13: MSE-minmax KATs over the (bits, num_attempts) matrix, generated from the reference.

Run:  python3 -B tests/golden/gen_f13_forms.py [--reference /root/reference]

Imports ``source.quantization`` from the read-only reference (no bytecode written) and
stores, per case of ``golden_cases.f13_cases()`` (inputs regenerated from numpy seeds), the
SHA-256 of the reference's ``quantize_tensor(x, bits, "tensor_mseminmax_symmetric",
num_attempts=na)`` and the candidate it chose (the index whose grid step reproduces the
output; recorded for the failure messages of the tests). Only data is written:
``f13_forms.json`` next to this script.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import golden_cases as gc  # noqa: E402

MSE = "tensor_mseminmax_symmetric"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from source import quantization as ref_quant  # noqa: E402
    torch.set_num_threads(1)
    meta = []
    for case in gc.f13_cases():
        x = torch.from_numpy(gc.f13_input(case).copy())
        y = ref_quant.quantize_tensor(x, case["bits"], MSE, num_attempts=case["num_attempts"])
        # the chosen candidate: the reference's own grid, quantized again candidate by candidate
        mx = torch.max(torch.abs(x.min()), torch.abs(x.max()))
        grid = torch.linspace(0.2 * mx.item(), 1.2 * mx.item(), case["num_attempts"])
        q = 2 ** (case["bits"] - 1)
        same = [i for i, t in enumerate(grid)
                if torch.equal(torch.clamp(torch.round(x / (2 * t / (2 * q - 1))), -q, q - 1) * (2 * t / (2 * q - 1)), y)]
        meta.append(dict(case, sha=gc.canonical_sha(y.numpy().astype(np.float32)), index=same[0] if same else None))
    with open(os.path.join(HERE, "f13_forms.json"), "w") as f:
        json.dump({"torch": torch.__version__, "threads": 1, "cases": meta}, f, indent=0)
    print(f"F13: {len(meta)} cases")


if __name__ == "__main__":
    main()
