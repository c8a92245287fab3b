"""The cases of tests/test_plan_digest.py and the generator of its fixture.

    python tests/golden/gen_plan_digests.py        # rewrites tests/golden/plan_digests.json

Every case is one call of admmq_debug_admm_plan_digest (eight FNV-1a digests of the ADMM
launch plan, one per section: scalars, descriptors, tiles, list offsets, sse / finalize
units, stage-1 units, thin units / teams / small jobs, device-table offsets) for a batch of
(I, R) factors under one setting of the planner's switches. The fixture was written by the
planner as it stood before it moved out of api.hip; it is regenerated only by a change that
means to alter a plan, never to make a refactor pass.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "plan_digests.json")
NCAND = 200
BASE = 1 << 20          # a fake workspace address: the planner never dereferences it
SECTIONS = ("scalars", "desc", "tiles", "list_off", "sse+fin", "hist+hist_multi", "thin+teams+small", "tables")

# resnet18's 16 3x3 convs, (I_0, I_1, R) (mode 2: I = 9) and one Llama-7B decoder layer,
# as tools/asan_host_check.c has them
R18 = [(64, 64, 134)] * 4 + [(128, 64, 183)] + [(128, 128, 278)] * 3 + [(256, 128, 375)] + [(256, 256, 566)] * 3 + \
      [(512, 256, 759)] + [(512, 512, 1141)] * 3
LLAMA = [(4096, 4096, 1024)] * 4 + [(11008, 4096, 1492)] * 2 + [(4096, 11008, 1492)]


def shape_sets():
    """name -> [(I, R), ...]: C3 / C4 / C5 per mode and the lone factors."""
    from admmq import synthetic
    sets = {}
    for m in range(3):
        sets[f"C3.mode{m}"] = [(9 if m == 2 else l[m], l[2]) for l in R18]
    for m in range(2):
        sets[f"C5.mode{m}"] = [(l[m], l[2]) for l in LLAMA]
    r50 = synthetic.resnet50_layers()
    for m in range(3):   # the 3x3 convs (3-way), the 1x1 layers (2-way), and the sweep's joint batch
        conv = [(s.shape[m], s.rank()) for s in r50 if len(s.shape) == 3]
        two = [(s.shape[m], s.rank()) for s in r50 if len(s.shape) == 2 and m < 2]
        both = [(s.shape[m], s.rank()) for s in r50 if len(s.shape) > m]
        sets[f"C4.conv3x3.mode{m}"] = conv
        if two:
            sets[f"C4.conv1x1.mode{m}"] = two
            sets[f"C4.all.mode{m}"] = both
    for i, r in ((512, 1141), (9, 1141), (17, 300)):
        sets[f"lone.{i}x{r}"] = [(i, r)]
    return sets


def random_sets(count=200):
    """The seeded batches of tools/asan_host_check.c (same xorshift64, same draw order):
    thin, 32-row, 64 x 64 and wide mixes, ragged R, R above 1152 in every 50th batch."""
    state = [88172645463325252]
    mask = (1 << 64) - 1

    def rnd(lo, hi):
        x = state[0]
        x ^= (x << 13) & mask
        x ^= x >> 7
        x ^= (x << 17) & mask
        state[0] = x
        return lo + x % (hi - lo + 1)

    sets = {}
    for t in range(count):
        n = rnd(1, 48)
        batch = []
        for _ in range(n):
            cls = rnd(0, 3)
            i = rnd(1, 16) if cls == 0 else rnd(17, 32) if cls == 1 else rnd(33, 700) if cls == 2 else rnd(700, 4096)
            batch.append((i, rnd(1, 3000 if t % 50 == 0 else 1200)))
        sets[f"random.{t:03d}"] = batch
    return sets


# name -> (setter, arguments, arguments that restore the default)
SETTINGS = {
    "ksplit=0": ("admmq_debug_set_ksplit", (0,), (1,)),
    "ksplit_form=0": ("admmq_debug_set_ksplit_form", (0,), (1,)),
    "ksplit_form=2": ("admmq_debug_set_ksplit_form", (2,), (1,)),
    "ksplit_balance=0,1": ("admmq_debug_set_ksplit_balance", (0, 1), (1, 1)),
    "ksplit_balance=1,4": ("admmq_debug_set_ksplit_balance", (1, 4), (1, 1)),
    "gemm_stage=2": ("admmq_debug_set_gemm_stage", (2,), (3,)),
    "gemm_ks=2": ("admmq_debug_set_gemm_ks", (2,), (1,)),
    "f32_persistent=1,1": ("admmq_debug_set_f32_persistent", (1, 1), (0, 1)),
    "f32_persistent=2,3": ("admmq_debug_set_f32_persistent", (2, 3), (0, 1)),
    "wide_min_tiles=0": ("admmq_debug_set_wide_min_tiles", (0,), (4 * 768,)),
    "even_units=0": ("admmq_debug_set_even_units", (0,), (1,)),
    "fin_nv3=0": ("admmq_debug_set_fin_nv3", (0,), (1,)),
    "thin_loop=2": ("admmq_debug_set_thin_loop", (2,), (1,)),
    "search_units_per_block=4": ("admmq_debug_set_search_units_per_block", (4,), (0,)),
    "solve=split": (None, (), ()),
}


def digest(lib, batch, solve_mode=0):
    from admmq import _lib
    arr = _lib.problems_array([_lib.AdmmProblem(0, 0, 0, 0, 0, 0, 0, i, r) for i, r in batch])
    out = (ctypes.c_uint64 * 8)()
    rc = lib.admmq_debug_admm_plan_digest(arr, len(batch), NCAND, solve_mode, ctypes.c_void_p(BASE), out)
    assert rc == 0, lib.admmq_last_error()
    return [f"{v:016x}" for v in out]


def cases(lib):
    """Yields (case name, first answer, second answer): every case is computed twice in a
    row (the tile memo's miss, then its hit). Default switches: every set; each setting of
    SETTINGS, one at a time: the C3 / C4 / C5 / lone sets."""
    named = shape_sets()
    for name, batch in {**named, **random_sets()}.items():
        yield f"default/{name}", digest(lib, batch), digest(lib, batch)
    for sname, (setter, args, restore) in SETTINGS.items():
        mode = 1 if setter is None else 0
        if setter:
            assert getattr(lib, setter)(*args) == 0, sname
        try:
            for name, batch in named.items():
                yield f"{sname}/{name}", digest(lib, batch, mode), digest(lib, batch, mode)
        finally:
            if setter:
                assert getattr(lib, setter)(*restore) == 0, sname


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    for p in (root, os.path.join(root, "admm-quantization_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from admmq import _lib
    lib = _lib.load()
    out = {}
    for name, first, second in cases(lib):
        assert first == second, name
        out[name] = first
    with open(FIXTURE, "w") as f:   # one case per line
        f.write(f'{{"sections": {json.dumps(SECTIONS)}, "num_attempts": {NCAND}, "digests": {{\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(out.items())))
        f.write("\n}}\n")
    print(f"{len(out)} cases -> {FIXTURE}")


if __name__ == "__main__":
    main()
