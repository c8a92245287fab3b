"""Every form of the ALS contraction kernels (csrc/als_kernels.hip) per element, off the layer
shapes: k_als_mttkrp<32 / 64> split and unsplit, k_als_mttkrp_sp<32 / 64, 9> in all three
modes, k_als_reduce, k_als_gram<32 / 64> with and without the Hadamard factor, and divmod at
the top of its range.

Every case of oracle.als_bound.CASES first asserts through the plan query
(admmq_debug_cp_plan, with W's real address) the form it is there for, then holds G and F of
every mode per element against the float64 contraction of the float32 inputs:

    |F - F64| <= (n_F + 4) 2^-24 BF        |G - G64| <= c_G 2^-24 BG

(derived in oracle/als_bound.py, nothing measured). W and the factors sit inside NaN guard
bands that must come back bit-unchanged, G is exactly symmetric, and a second call returns the
same bits. Each case prints its worst ratio err / (2^-24 B) beside the constant. At the top
of divmod's range, where that bound is as large as BF, integer-valued inputs add an exact check.
"""
import numpy as np
import pytest

from conftest import gpu_available
from oracle import als_bound as ab

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

JOB = {ab.GENERIC: "generic", ab.SPATIAL: "spatial"}


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def _place(torch, dev, W, fs, band):
    views, bufs = zip(*[ab.banded(torch, dev, a, band) for a in [W] + list(fs)])
    return views[0], list(views[1:]), bufs, [b.clone() for b in bufs]


def _unchanged(torch, bufs, before):
    for b, b0 in zip(bufs, before):   # bands and operands, bit for bit (NaN payloads included)
        assert torch.equal(b.view(torch.int32), b0.view(torch.int32))


def _check_mode(torch, dims, R, mode, Wd, fd, ref, want_plan, tag):
    """Plan, two calls, the per-element bounds. Returns (G, F) of the first call."""
    from admmq import _lib
    from admmq.als import gram_mttkrp
    plan = _lib.debug_cp_plan([(dims, R, Wd.data_ptr())], mode)[0]
    assert {k: plan[k] for k in want_plan} == want_plan, (dims, R, mode, plan)
    gplan = _lib.debug_cp_plan([(dims, R, Wd.data_ptr())], mode, "gram")[0]
    assert gplan["job"] == ab.GRAM and gplan["BM"] == (32 if R <= 32 else 64)
    G, F = gram_mttkrp(Wd, fd, mode)
    G2, F2 = gram_mttkrp(Wd, fd, mode)
    G64, F64, BG, BF = ref
    rf, rg = ab.worst_ratio(F.cpu().numpy(), F64, BF), ab.worst_ratio(G.cpu().numpy(), G64, BG)
    cf, cg = ab.f_constant(dims, mode), ab.g_constant(dims, mode)
    form = f"{JOB[plan['job']]}<{plan['BM']}> mode {mode}" + (f" nsplit {plan['nsplit']}" if plan["nsplit"] > 1 else "")
    print(f"FORM {tag} {dims} R={R} | {form} | F worst err / (2^-24 BF) = {rf:.3f} of c = {cf:.0f} | "
          f"gram<{gplan['BM']}>{' hadamard' if len(dims) == 3 else ''} | G {rg:.3f} of c = {cg:.0f}")
    assert tuple(F.shape) == (dims[mode], R) and tuple(G.shape) == (R, R)
    assert rf <= cf, (dims, R, mode, rf, cf)
    assert rg <= cg, (dims, R, mode, rg, cg)
    assert torch.equal(G, G.T), "Gram product must be exactly symmetric"
    assert torch.equal(G.view(torch.int32), G2.view(torch.int32)) and torch.equal(F.view(torch.int32), F2.view(torch.int32))
    return G, F


@pytest.mark.parametrize("case", ab.CASES, ids=ab.case_id)
def test_form_per_element(torch_dev, case):
    torch, dev = torch_dev
    dims, R, band = case["dims"], case["R"], case["band"]
    W, fs = ab.case_inputs(dims, R)
    Wd, fd, bufs, before = _place(torch, dev, W, fs, band)
    out = [_check_mode(torch, dims, R, m, Wd, fd, ab.case_reference(dims, R, m), case["plan"][m], "case")
           for m in range(len(dims))]
    _unchanged(torch, bufs, before)
    if band % 4:   # the misaligned call against the aligned one: another kernel, another summation order
        Wa, fa, bufs_a, before_a = _place(torch, dev, W, fs, 64)
        from admmq import _lib
        from admmq.als import gram_mttkrp
        for m, (G, F) in enumerate(out):
            assert _lib.debug_cp_plan([(dims, R, Wa.data_ptr())], m)[0]["job"] == ab.SPATIAL
            Ga, Fa = gram_mttkrp(Wa, fa, m)
            G64, F64, BG, BF = ab.case_reference(dims, R, m)
            assert ab.worst_ratio(Fa.cpu().numpy(), F64, BF) <= ab.f_constant(dims, m)
            assert torch.equal(G, Ga)
            assert not torch.equal(F, Fa), f"mode {m}: the generic and the spatial form agree bit for bit"
        _unchanged(torch, bufs_a, before_a)


def test_top_of_divmod_range(torch_dev):
    """K just below 2^24: divisor 3 (the down-correction on a third of the range) and J in
    (1, 5592403, 3), divisor 4099 in (4093, 4099, 2); the same per-element bound against a
    float64 contraction formed mode by mode (no (I, J, R) intermediate)."""
    torch, dev = torch_dev
    for dims, R, plans in ab.TOP:
        g = np.random.default_rng(sum(dims))
        fs = [g.standard_normal((n, R), dtype=np.float32) for n in dims]
        W = g.standard_normal(dims, dtype=np.float32)
        Wd, fd, bufs, before = _place(torch, dev, W, fs, 64)
        for m, (nsplit, kchunk) in plans.items():
            want = dict(job=ab.GENERIC, BM=32, nsplit=nsplit, kchunk=kchunk)
            _check_mode(torch, dims, R, m, Wd, fd, ab.reference(W, fs, m), want, "top")
        _unchanged(torch, bufs, before)
        del Wd, fd, bufs, before
        # n_F 2^-24 is about 1 here, so the bound above is nearly as large as BF itself and a few
        # wrong Khatri-Rao indices would pass it. Entries in {-1, 0, 1} close that: every product is
        # -1, 0 or 1 and BF, the count of non-zero products, is below 2^24, so every partial sum in
        # any order is an integer float32 holds exactly - F must equal the float64 sum, digit for digit.
        fs = [g.integers(-1, 2, (n, R), dtype=np.int8).astype(np.float32) for n in dims]
        W = g.integers(-1, 2, dims, dtype=np.int8).astype(np.float32)
        Wd, fd, bufs, before = _place(torch, dev, W, fs, 64)
        from admmq.als import gram_mttkrp
        for m in plans:
            _, F64, _, BF = ab.reference(W, fs, m)
            assert 0 < BF.max() < 2 ** 24
            F = gram_mttkrp(Wd, fd, m)[1].cpu().numpy()
            print(f"FORM top {dims} R={R} mode {m} integer entries: |F| <= {np.abs(F64).max():.0f}, BF <= {BF.max():.0f}, "
                  f"max |F - F64| = {np.abs(F - F64).max():.0f}")
            assert np.array_equal(F.astype(np.float64), F64), (dims, m)
        _unchanged(torch, bufs, before)
        del Wd, fd, bufs, before


@pytest.mark.parametrize("route", ["ops", "ctypes"])
def test_mixed_batch_equals_single(torch_dev, route, monkeypatch):
    """One batch with both BM classes, both MTTKRP kernels, split and unsplit jobs, 2-way and
    3-way, forwards and reversed (the unit offsets per launch and the split ids): every (G, F)
    bit-equal to its single call, through torch.ops and through the C-ABI."""
    torch, dev = torch_dev
    from admmq import _lib
    from admmq.als import gram_mttkrp, gram_mttkrp_batched
    if route == "ctypes":
        monkeypatch.setattr(_lib, "use_ops", lambda: False)
    layers = []
    for dims, R in ab.MIXED:
        W, fs = ab.case_inputs(dims, R)
        layers.append((torch.from_numpy(W).to(dev), [torch.from_numpy(f).to(dev) for f in fs]))
    for mode in range(3):
        sel = [L for L in layers if mode < L[0].dim()]
        plans = _lib.debug_cp_plan([(tuple(W.shape), fs[0].shape[1], W.data_ptr()) for W, fs in sel], mode)
        assert {p["job"] for p in plans} == {ab.GENERIC, ab.SPATIAL} and {p["BM"] for p in plans} == {32, 64}
        single = [gram_mttkrp(W, fs, mode) for W, fs in sel]
        for (W, fs), (G, F) in zip(sel, single):
            G64, F64, BG, BF = ab.case_reference(tuple(W.shape), fs[0].shape[1], mode)
            assert ab.worst_ratio(F.cpu().numpy(), F64, BF) <= ab.f_constant(tuple(W.shape), mode)
            assert ab.worst_ratio(G.cpu().numpy(), G64, BG) <= ab.g_constant(tuple(W.shape), mode)
        for order in (slice(None), slice(None, None, -1)):
            batch = gram_mttkrp_batched(sel[order], mode)
            assert len(batch) == len(sel)
            for (G, F), (Gs, Fs) in zip(batch, single[order]):
                assert torch.equal(G.view(torch.int32), Gs.view(torch.int32))
                assert torch.equal(F.view(torch.int32), Fs.view(torch.int32))
