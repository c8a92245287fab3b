"""The solve GEMM's launch head (admmq_debug_set_launch_head).

Bit 0 moves the loads of the stop test's inputs (the problem's flag and the previous
iteration's residual sums) from behind the problem descriptor to the tile record, beside the
first ring stages, and takes the decision at the first K-step's wait. The float operations
and their order are unchanged, so every case here runs the same inputs with mask 0 (the
descriptor-chain head) and with the library's default mask and requires identical bits: H, U,
the last H_T, and info (iterations run, stop flag, SPD flag, fault flag).

The early-exit problems are G = B B^T + c I with the ridge c chosen per problem so that the
reference (oracle/admm_oracle.py) stops at distinct iterations for one eps: at eps = 0.3,
(40, 70) c = 4 stops at 6, (64, 134) c = 0.5 at 8, (128, 183) c = 0.08 at 13, each with the
stop test's max(r, s) at least 12 % away from eps on both sides of the stop (measured on the
CPU with the oracle before the cases were fixed), so the device's fp32-inverse solve cannot
tip the comparison."""
import ctypes

import numpy as np
import pytest

from conftest import gpu_available
from oracle import admm_oracle as ao

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE = "tensor_mseminmax_symmetric"
EPS = 0.3
# (I, R, seed, ridge): the reference's stop iteration at EPS is 6, 8, 13 (see above)
EARLY = [(40, 70, 7, 4.0), (64, 134, 7, 0.5), (128, 183, 9, 0.08)]
KSPLIT = (256, 566, 7, 0.5)    # np = 3, 36 tiles: parallel pieces when alone in its launch
WIDE = (256, 300, 7, 0.5)


def _problem(I, R, seed, ridge):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((R, 2 * R)) / np.sqrt(2 * R)
    G = (B @ B.T + ridge * np.eye(R)).astype(np.float32)
    F = rng.standard_normal((I, R)).astype(np.float32)
    H = (rng.standard_normal((I, R)) * 0.1).astype(np.float32)
    return H, F, G


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def oracle_stops():
    """The reference's iteration counts of the early-exit problems (computed once)."""
    out = {}
    for spec in EARLY + [KSPLIT, WIDE]:
        H, F, G = _problem(*spec)
        _, _, info = ao.admm_iteration(H, np.zeros_like(H), F, G, 40, EPS, 4, MSE, return_info=True)
        out[spec] = info["iters"]
    return out


class _head:
    """The launch-head mask held for a block (None: the library's default)."""

    def __init__(self, mask):
        from admmq import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.default = self.lib.admmq_debug_get_launch_head_default()
        self.mask = self.default if mask is None else mask

    def __enter__(self):
        self._lib.check(self.lib.admmq_debug_set_launch_head(self.mask), "launch_head")
        return self

    def __exit__(self, *exc):
        self._lib.check(self.lib.admmq_debug_set_launch_head(self.default), "launch_head")
        return False


def _run(torch_dev, specs, max_iter, eps, mask, repeat=1, **kw):
    """[(H, U, H_T)] per problem and info, of `repeat` calls on the same tensors' fresh copies
    (the workspace is the allocator's: the same block again for the same sizes)."""
    torch, dev = torch_dev
    from admmq import admm_iteration_batched
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    outs = []
    with _head(mask):
        for _ in range(repeat):
            ps = [(t(H), torch.zeros(H.shape, device=dev), t(F), t(G)) for H, F, G in (_problem(*s) for s in specs)]
            if max_iter <= 1:
                Hs, info = admm_iteration_batched(ps, max_iter, eps, 4, MSE, return_info=True, **kw)
                dbg = [(h, h) for h in Hs]
            else:
                Hs, dbg, info = admm_iteration_batched(ps, max_iter, eps, 4, MSE, debug_outputs=True, return_info=True,
                                                       **kw)
            outs.append(([(h.cpu(), p[1].cpu(), d[0].cpu()) for h, p, d in zip(Hs, ps, dbg)], info.cpu()))
    return outs


def _same(torch, a, b):
    (ra, ia), (rb, ib) = a, b
    assert torch.equal(ia, ib), (ia, ib)
    for x, y in zip(ra, rb):
        for u, v in zip(x, y):
            assert torch.equal(u, v)


def _default_differs():
    from admmq import _lib
    return _lib.load().admmq_debug_get_launch_head_default() != 0


def test_setter_range():
    from admmq import _lib
    lib = _lib.load()
    d = lib.admmq_debug_get_launch_head_default()
    assert d == 1   # the kept parts: bit 0
    assert lib.admmq_debug_set_launch_head(-1) != 0 and lib.admmq_debug_set_launch_head(2) != 0
    assert lib.admmq_debug_set_launch_head(0) == 0 and lib.admmq_debug_set_launch_head(d) == 0


def test_early_exit_serial_tiles_batch(torch_dev, oracle_stops):
    """Three problems in one batch that stop at distinct iterations, all below 40."""
    torch, _ = torch_dev
    want = [oracle_stops[s] for s in EARLY]
    print("oracle stops", want)
    assert len(set(want)) == 3 and max(want) < 39
    a = _run(torch_dev, EARLY, 40, EPS, 0)[0]
    b = _run(torch_dev, EARLY, 40, EPS, None)[0]
    print("device iterations: mask 0", a[1][:, 0].tolist(), "default", b[1][:, 0].tolist())
    assert _default_differs()
    _same(torch, a, b)
    assert b[1][:, 0].tolist() == want and b[1][:, 1].tolist() == [1, 1, 1]
    assert (b[1][:, 2:4] == 0).all()


@pytest.mark.parametrize("max_iter", [1, 2])
def test_shortest_calls(torch_dev, max_iter):
    torch, _ = torch_dev
    _same(torch, _run(torch_dev, EARLY, max_iter, EPS, 0)[0], _run(torch_dev, EARLY, max_iter, EPS, None)[0])


def test_early_exit_parallel_ksplit(torch_dev, oracle_stops):
    """A lone (256, 566) factor: parallel K-split pieces. Twice on one workspace: a skipped
    iteration must leave the tiles' arrival counters consistent for the next call."""
    torch, _ = torch_dev
    from admmq import _lib
    assert _lib.load().admmq_debug_ksplit_pieces(256, 566) == 3
    want = oracle_stops[KSPLIT]
    assert want < 39
    a = _run(torch_dev, [KSPLIT], 40, EPS, 0, repeat=2)
    b = _run(torch_dev, [KSPLIT], 40, EPS, None, repeat=2)
    print("oracle", want, "device", [x[1][0, 0].item() for x in a + b])
    for x in a + b:
        assert x[1][0, 0].item() == want and x[1][0, 1].item() == 1 and (x[1][0, 2:4] == 0).all()
    _same(torch, a[0], b[0])
    _same(torch, a[1], b[1])
    _same(torch, b[0], b[1])
    _same(torch, _run(torch_dev, [KSPLIT], 9, 0.0, 0)[0], _run(torch_dev, [KSPLIT], 9, 0.0, None)[0])


@pytest.mark.parametrize("form,eps,iters", [("wide", 0.0, 7), ("wide", EPS, 40), ("split", 0.0, 7)])
def test_wide_and_split_forms(torch_dev, oracle_stops, form, eps, iters):
    """k_gemm's wide tiles (forced by a zero threshold) and its split operand form."""
    torch, _ = torch_dev
    from admmq import _lib
    lib = _lib.load()
    kw = {"solve": "split"} if form == "split" else {}
    if form == "wide":
        _lib.check(lib.admmq_debug_set_wide_min_tiles(0), "wide_min_tiles")
    try:
        a = _run(torch_dev, [WIDE], iters, eps, 0, **kw)[0]
        b = _run(torch_dev, [WIDE], iters, eps, None, **kw)[0]
    finally:
        _lib.check(lib.admmq_debug_set_wide_min_tiles(4 * 768), "wide_min_tiles")
    _same(torch, a, b)
    if eps > 0:
        assert b[1][0, 0].item() == oracle_stops[WIDE] < 39
    else:
        assert b[1][0, 0].item() == iters - 1


@pytest.mark.parametrize("search", ["fused", "separate", "exhaustive"])
def test_search_forms_beside_the_moved_stop_test(torch_dev, search):
    """A batch with a job of one search block and a job of many, under each search form: the
    search reads the flag the solve's moved branch sets."""
    torch, _ = torch_dev
    from admmq import _lib
    specs = [(24, 40, 3, 0.5), KSPLIT]

    def run(mask):
        with _lib.fused_finalize(search == "fused"), _lib.exhaustive_search(search == "exhaustive"):
            return _run(torch_dev, specs, 5, 0.0, mask)[0]

    _same(torch, run(0), run(None))


def test_quantize_batched_unaffected(torch_dev):
    torch, dev = torch_dev
    from admmq import quantize_batched
    xs = [torch.from_numpy(_problem(*s)[1]).to(dev) for s in [(24, 40, 3, 0.5), KSPLIT]]
    with _head(0):
        a = quantize_batched(xs, 4, MSE)
    with _head(None):
        b = quantize_batched(xs, 4, MSE)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_no_wasted_work_after_the_break(torch_dev, oracle_stops):
    """The GEMM class average of a call that broke at iteration 8 of 400 must stay that of
    launches that end at the stop test: a K-loop run on the skipped launches would multiply
    it. The bound between the two heads is a factor 2, either way."""
    torch, dev = torch_dev
    from admmq import _lib, admm_iteration_batched
    lib = _lib.load()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    specs = [KSPLIT, WIDE]   # together: serial pieces, 18 K-steps per tile of the larger factor
    want = [oracle_stops[s] for s in specs]
    assert max(want) < 39
    avg = {}
    for mask in (0, None):
        with _head(mask):
            for rep in range(2):   # the first call warms the allocator and the code objects
                p = [(t(H), torch.zeros(H.shape, device=dev), t(F), t(G)) for H, F, G in (_problem(*s) for s in specs)]
                torch.cuda.synchronize()
                _lib.check(lib.admmq_profile_begin(2048, 1), "profile_begin")
                _, info = admm_iteration_batched(p, 400, EPS, 4, MSE, return_info=True)
                ms = (ctypes.c_double * 8)()
                cnt = (ctypes.c_int64 * 8)()
                _lib.check(lib.admmq_profile_end(ms, cnt), "profile_end")
                assert info[:, 0].tolist() == want and cnt[0] == 399
                avg[mask] = 1e3 * ms[0] / cnt[0]
    print("GEMM class average us per launch: mask 0 %.2f, default %.2f" % (avg[0], avg[None]))
    assert avg[None] < 2 * avg[0] and avg[0] < 2 * avg[None]
