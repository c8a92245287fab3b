"""Golden fixture F12: the reference's own fixed-range activation quantizers.

    python tests/golden/gen_f12_actquant.py --reference /path/to/reference

imports ``source.quantization`` of the reference checkout (third-party packages it does not need
here are stubbed, as gen_golden.py does) and writes ``f12_actquant.npz`` / ``.json`` beside this
file: inputs from seeds, and the bits (uint32 views) of what ``min_max_quantize``,
``fixed_quantize``, ``MinMaxQuant`` and ``MovingAvgMinMaxQuant`` return on the CPU. Data only.
"""
import argparse
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
BITS = [1, 2, 4, 8, 16]
RANGES = [(0.3, 1.4), (-1.7, 1.6), (0.5, 0.5), (0.5, -1.5)]   # (min, max): the last two have rng == 0 and rng < 0
BOUNDARY_RANGES = [(0.3, 1.1), (-1.7, 3.3), (0.013, 0.77)]    # (mn, rng): no rng is a power of two


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: (_ for _ in ()).throw(RuntimeError(f"stubbed {self.__name__}.{name}"))


def import_reference(path):
    for m in ["tensorly", "tensorly.decomposition", "tensorly.decomposition.candecomp_parafac", "tensorly.kruskal_tensor",
              "musco", "musco.pytorch", "musco.pytorch.compressor", "musco.pytorch.compressor.decompose",
              "musco.pytorch.compressor.decompose.cpd", "musco.pytorch.compressor.decompose.cpd.lib_anc"]:
        sys.modules.setdefault(m, _Stub(m))
    sys.path.insert(0, path)
    from source import quantization as ref_quant
    return ref_quant


def bits_of(t):
    return t.detach().to(torch.float32).contiguous().numpy().view(np.uint32).copy()


def inputs():
    g = torch.Generator().manual_seed(1212)
    out = {}
    for n in (1, 7, 4099):
        x = torch.randn(n, generator=g) * 2.0
        out[f"clean{n}"] = x.clone()
        sp = [float("nan"), float("inf"), -float("inf"), -0.0, 1e30, -1e30, 1e-40]
        if n == 1:
            x[0] = -0.0
        else:
            for i, v in enumerate(sp):
                x[(i * 13) % n if n > 7 else i] = v
        out[f"x{n}"] = x
    return out


def f32(v):
    return float(np.float32(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    a = ap.parse_args()
    rq = import_reference(a.reference)
    arrays, cases = {}, []
    xs = inputs()
    for k, v in xs.items():
        arrays["in_" + k] = v.numpy()
    one, zero = torch.ones(1), torch.zeros(1)

    def add(cid, y, **rec):
        arrays["out_" + cid] = bits_of(y)
        cases.append(dict(id=cid, **rec))

    # ---- function cases
    for bits in BITS:
        for n in (1, 7, 4099):
            x = xs[f"x{n}"]
            for ri, (lo, hi) in enumerate(RANGES if n < 4099 else RANGES[:1]):
                lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
                routes = dict(tensor=(lo32, hi32), float=(lo, hi), mixed_tf=(lo32, hi), mixed_ft=(lo, hi32))
                for route, (p, q) in routes.items():
                    if n == 4099 and route != "tensor":   # (the fixture's size: the routes differ in (mn, rng) only)
                        continue
                    y = rq.min_max_quantize(x.clone(), bits, p, q)
                    # the (mn, rng) that torch's own promotion gives the reference's expressions
                    mn, rng = float((zero + p)[0]), float((one * (q - p))[0])
                    add(f"mm_{route}_b{bits}_n{n}_r{ri}", y, kind="min_max", route=route, bits=bits, input=f"x{n}",
                        min=f32(lo) if route in ("tensor", "mixed_tf") else lo,
                        max=f32(hi) if route in ("tensor", "mixed_ft") else hi, mn=mn, rng=rng)
                zp, sc = lo, hi - lo
                y = rq.fixed_quantize(x.clone(), bits, zp, sc)
                add(f"fx_b{bits}_n{n}_r{ri}", y, kind="fixed", bits=bits, input=f"x{n}", zero_point=zp, scope=sc)
            if n > 1:
                xc = xs[f"clean{n}"]
                add(f"mm_none_b{bits}_n{n}", rq.min_max_quantize(xc.clone(), bits, None, 1.0), kind="one_none", bits=bits,
                    input=f"clean{n}")
    for ri, (lo, hi) in enumerate(RANGES[2:], 2):   # rng == 0 and rng < 0 at the large size
        y = rq.fixed_quantize(xs["x4099"].clone(), 4, lo, hi - lo)
        add(f"fx_b4_n4099_r{ri}", y, kind="fixed", bits=4, input="x4099", zero_point=lo, scope=hi - lo)

    # ---- boundary cases: the half-way point of every level moved by -2..+2 ulps
    for bits, levels in ((4, 15), (8, 64)):
        n = 2 ** bits - 1
        for ri, (mn, rng) in enumerate(BOUNDARY_RANGES):
            mn32, rng32 = np.float32(mn), np.float32(rng)
            js = np.arange(n, dtype=np.float64) if levels >= n else np.linspace(0, n - 1, levels).round()
            mid = (np.float64(mn32) + (js + 0.5) * np.float64(rng32) / n).astype(np.float32)
            parts = []
            for d in (-2, -1, 0, 1, 2):
                v = mid.copy()
                for _ in range(abs(d)):
                    v = np.nextafter(v, np.float32(np.inf if d > 0 else -np.inf), dtype=np.float32)
                parts.append(v)
            x = torch.from_numpy(np.concatenate(parts))
            cid = f"bd_b{bits}_r{ri}"
            arrays["in_" + cid] = x.numpy()
            add(cid, rq.fixed_quantize(x.clone(), bits, float(mn32), float(rng32)), kind="boundary", bits=bits,
                input=cid, zero_point=float(mn32), scope=float(rng32))

    # ---- observers: four batches [2, 3, 4, 4], counter 6: three observed, the fourth quantized
    g = torch.Generator().manual_seed(1213)
    batches = [torch.randn(2, 3, 4, 4, generator=g) * (1.0 + 0.5 * i) for i in range(4)]
    arrays["in_obs"] = torch.stack(batches).numpy()
    for ltype in ("minmax", "avgminmax"):
        q = rq.get_quant_layer(ltype, "s", bits=8, counter=6)
        stats = []
        for b in batches[:3]:
            out = q(b.clone())
            assert out is not None and torch.equal(out, b)
            stats.append([int(bits_of(q.min_val.reshape(1))[0]), int(bits_of(q.max_val.reshape(1))[0])])
        assert q.counter == 0
        add(f"obs_{ltype}", q(batches[3].clone()), kind="observer", ltype=ltype, bits=8, counter=6, stats_bits=stats)

    np.savez_compressed(os.path.join(HERE, "f12_actquant.npz"), **arrays)
    with open(os.path.join(HERE, "f12_actquant.json"), "w") as f:
        json.dump(dict(fixture="f12_actquant", cases=cases), f, indent=0)
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
