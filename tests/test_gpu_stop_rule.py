"""The stop rule (source/admm.py:62-65: break when r < eps and s < eps) of every device path
against the reference's iteration count at a deciding eps.

The rule has five device copies (converged_before, stop_load / stop_test, the split k_gemm
head, k_thin_solve, k_thin_loop) fed by residual sums formed in four places (k_finalize_admm,
the fused finalize of k_mse_hist3, k_mse_small_admm, the thin loop's finalize). The cases
(oracle/solve_bound.py STOP_BATCHES) are batches of three problems G = B B^T + ridge I,
U0 = 0, that the reference stops at three distinct iterations <= 8 for the batch's one eps,
with max(r, s) of every iteration up to the stop at least 25 % away from eps
(tests/test_solve_bound_host.py asserts that from the oracle's history), so neither the
device's fp32 inverse nor its float32 partial squares can decide.

Each path must show:
  * info[:, 0] equal to the oracle's iteration counts and info[:, 1] == 1;
  * the sticky break: a stopped problem's H and U equal, bit for bit, those of the same call
    with eps = 0 and max_iter = stop + 1 - nothing is written after the break;
  * independence: every problem equals its own single call, whatever stopped beside it;
  * the last iteration: with max_iter - 1 equal to a problem's stop iteration the reference
    breaks there, but nothing on the device tests after the last finalize: iterations run =
    max_iter - 1, H and U equal the eps = 0 run, and info[:, 1] reports 0 for that problem
    (include/admmq.h says so): "converged" means a later iteration was skipped.
"""
import contextlib

import numpy as np
import pytest

from conftest import gpu_available
from oracle import solve_bound as sb

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def oracle_stops():
    """The reference's iteration counts per batch, computed once on demand."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = [sb.stop_history(name, k)[0] for k in range(3)]
        return cache[name]
    return get


@contextlib.contextmanager
def _setter(name, value, restore):
    from admmq import _lib
    fn = getattr(_lib.load(), name)
    args = lambda v: v if isinstance(v, tuple) else (v,)  # noqa: E731
    try:
        _lib.check(fn(*args(value)), name)
        yield
    finally:
        _lib.check(fn(*args(restore)), name)


def _thin_loop(mode):
    from admmq import _lib
    return _lib.thin_loop(mode)


@contextlib.contextmanager
def _separate_finalize(units):
    from admmq import _lib
    with _lib.fused_finalize(False), _lib.search_units_per_block(units):
        yield


def _launch_head0():
    from admmq import _lib
    return _setter("admmq_debug_set_launch_head", 0, _lib.load().admmq_debug_get_launch_head_default())


# launch classes of admmq_profile_end (include/admmq.h ADMMQ_PROF_*)
_GEMM, _GEMM_THIN, _SEARCH, _SMALL, _FINALIZE, _THIN_LOOP = 0, 1, 2, 3, 4, 6

# id -> (batch, context factory, solve form)
PATHS = {
    "thin_loop": ("thin", lambda: _thin_loop(True), None),
    "thin_loop_wide": ("thin", lambda: _thin_loop("wide"), None),
    "thin_per_iteration": ("thin", lambda: _thin_loop(False), None),
    "mixed_default": ("mixed", contextlib.nullcontext, None),
    "mixed_separate_finalize_1": ("mixed", lambda: _separate_finalize(1), None),
    "mixed_separate_finalize_8": ("mixed", lambda: _separate_finalize(8), None),
    "mixed_split": ("mixed", contextlib.nullcontext, "split"),
    "mixed_f32p": ("mixed", lambda: _setter("admmq_debug_set_f32_persistent", (1, 1), (0, 1)), None),
    "mixed_f32t": ("mixed", lambda: _setter("admmq_debug_set_f32_persistent", (2, 1), (0, 1)), None),
    "mixed_launch_head_0": ("mixed", _launch_head0, None),
    "mixed_minmax": ("minmax", contextlib.nullcontext, None),
    "mixed_symmetric": ("symmetric", contextlib.nullcontext, None),
    "mixed_affine": ("affine", contextlib.nullcontext, None),
}


def _call(torch_dev, name, max_iter, eps, solve, only=None, counts=None):
    """([(H, U)] per problem in numpy, info[:, :2]) of one call on fresh copies of batch
    `name` (`only`: that problem alone; `counts`: a list that receives the call's launch
    counts per class)."""
    import ctypes
    torch, dev = torch_dev
    from admmq import admm_iteration_batched, _lib
    lib = _lib.load()
    scheme, _, specs, _ = sb.STOP_BATCHES[name]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ps = []
    for k, spec in enumerate(specs):
        if only is None or k == only:
            H, F, G = sb.stop_problem(*spec)
            ps.append((t(H), torch.zeros(H.shape, device=dev), t(F), t(G)))
    ms, cnt = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)()
    if counts is not None:
        _lib.check(lib.admmq_profile_begin(256, 1), "profile_begin")
    try:
        Hs, info = admm_iteration_batched(ps, max_iter, eps, 4, scheme, return_info=True, solve=solve)
        torch.cuda.synchronize()
    finally:
        if counts is not None:
            _lib.check(lib.admmq_profile_end(ms, cnt), "profile_end")
            counts.extend(int(c) for c in cnt)
    info = info.cpu().numpy()
    assert (info[:, 2:] == 0).all(), info   # no SPD error, no internal fault, no re-run
    return [(H.cpu().numpy(), p[1].cpu().numpy()) for H, p in zip(Hs, ps)], info[:, :2]


def _equal(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("path", list(PATHS))
def test_stop_iteration_matches_oracle(torch_dev, oracle_stops, path):
    name, ctx, solve = PATHS[path]
    eps = sb.stop_eps(name)
    want = oracle_stops(name)
    assert want == sb.STOP_BATCHES[name][3] and len(set(want)) == 3 and max(want) <= 8
    with ctx():
        cnt = []
        got, info = _call(torch_dev, name, sb.STOP_MAX_ITER, eps, solve, counts=cnt)
        print(f"{path}: oracle stops {want}, device info {info.tolist()}, launches per class {cnt}")
        # the path ran: the loop alone, or the per-iteration thin solve with the one-block
        # search + finalize, or the MFMA solve beside the thin one with a finalize of its own
        per_iter = sb.STOP_MAX_ITER - 1
        if path.startswith("thin_loop"):
            assert cnt[_THIN_LOOP] == 1 and cnt[_GEMM] == cnt[_GEMM_THIN] == cnt[_SMALL] == cnt[_FINALIZE] == 0, cnt
        elif path == "thin_per_iteration":
            assert cnt[_THIN_LOOP] == 0 and cnt[_GEMM] == 0 and cnt[_GEMM_THIN] == cnt[_SMALL] == per_iter, cnt
        else:
            assert cnt[_THIN_LOOP] == 0 and cnt[_GEMM] == cnt[_GEMM_THIN] == per_iter, cnt
            if "separate_finalize" in path:
                assert cnt[_FINALIZE] == per_iter, cnt
        assert info[:, 0].tolist() == want
        assert info[:, 1].tolist() == [1, 1, 1]
        for k, stop in enumerate(want):
            # the sticky break: nothing is written after it
            ref, ri = _call(torch_dev, name, stop + 1, 0.0, solve)
            assert ri[k].tolist() == [stop, 0]
            assert _equal(got[k], ref[k]), (path, k, "differs from eps = 0, max_iter = stop + 1")
            # a problem is unaffected by the breaks beside it
            alone, ai = _call(torch_dev, name, sb.STOP_MAX_ITER, eps, solve, only=k)
            assert ai[0].tolist() == [stop, 1]
            assert _equal(got[k], alone[0]), (path, k, "differs from its single call")


@pytest.mark.parametrize("path", list(PATHS))
def test_rule_met_at_the_last_iteration(torch_dev, oracle_stops, path):
    """max_iter - 1 is the middle problem's stop iteration: the earliest problem broke before
    (converged 1), the middle one meets the rule in the last iteration run (nothing tests
    after the last finalize: converged 0), the latest has not met it (converged 0)."""
    name, ctx, solve = PATHS[path]
    eps = sb.stop_eps(name)
    want = oracle_stops(name)
    last = sorted(want)[1]
    with ctx():
        got, info = _call(torch_dev, name, last + 1, eps, solve)
        ref, ri = _call(torch_dev, name, last + 1, 0.0, solve)
    print(f"{path}: max_iter {last + 1}, oracle stops {want}, device info {info.tolist()}")
    assert info[:, 0].tolist() == [min(w, last) for w in want]
    assert info[:, 1].tolist() == [1 if w < last else 0 for w in want]
    assert ri.tolist() == [[last, 0]] * 3
    for k, w in enumerate(want):
        if w >= last:
            assert _equal(got[k], ref[k]), (path, k)
