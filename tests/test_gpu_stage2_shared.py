"""The fused search launch's stage 2 shared among a job's blocks (k_mse_hist3, FIN): when the
selection leaves more than one candidate, the last block publishes the record first and every
block of the job adds the canonical SSE terms of its own quads; a second arrival on the job's
ticket word orders the sums before the argmin. The terms are integers, so the bits must equal
the one-block sweep of the separate-finalize path, whatever the selected set is."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE = "tensor_mseminmax_symmetric"
# non-thin factors (I > 16): 1 block, a few blocks, 9 blocks with a partial last unit, one layer4 shape
SHAPES = [(20, 134), (64, 278), (128, 566), (512, 1141)]


def _problems(torch, dev, shapes, seed, ridge=0.05):
    """(H0, F, G) per shape on the device: G = A^T A / m + ridge I (SPD), F = H* G + noise."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for I, R in shapes:
        A = torch.randn(R + 32, R, generator=g).to(dev)
        G = (A.T @ A) / (R + 32) + ridge * torch.eye(R, device=dev)
        Hs = torch.randn(I, R, generator=g).to(dev)
        F = Hs @ G + 0.01 * torch.randn(I, R, generator=g).to(dev)
        H0 = torch.randn(I, R, generator=g).to(dev)
        out.append((H0.contiguous(), F.contiguous(), G.contiguous()))
    torch.cuda.synchronize()
    return out


def _run(torch, probs, iters, eps, widen, fused):
    """One batched call; returns ([(H bytes, U bytes)], info, shared-stage-2 count of the call)."""
    from admmq import admm_iteration_batched
    from admmq import _lib
    import contextlib
    ps = [(H.clone(), torch.zeros_like(H), F, G) for H, F, G in probs]
    _lib.shared_stage2_count(reset=True)
    with contextlib.ExitStack() as st:
        if widen:
            st.enter_context(_lib.sel_widen(widen))
        st.enter_context(_lib.fused_finalize(fused))
        Hs, info = admm_iteration_batched(ps, iters, eps, 4, MSE, return_info=True)
    torch.cuda.synchronize()
    count = _lib.shared_stage2_count(reset=True)
    info = info.cpu().numpy()
    outs = [(h.cpu().numpy().tobytes(), p[1].cpu().numpy().tobytes()) for h, p in zip(Hs, ps)]
    return outs, info, count


def _six_runs(torch, probs, iters, eps):
    """default / sel_widen 1 / sel_widen 2, each with the fused finalize on and off: the bits
    agree, no fault, and under a widened selection the fused runs' shared stage 2 ran once per
    job and iteration (a run that silently took the single-candidate path fails here)."""
    from admmq import _lib
    _lib.fault_repairs(reset=True)
    ref = None
    infos = {}
    for widen in (0, 1, 2):
        for fused in (True, False):
            outs, info, count = _run(torch, probs, iters, eps, widen, fused)
            print(f"widen {widen} fused {fused}: shared stage 2 count {count}, iterations {info[:, 0].tolist()}, "
                  f"converged {info[:, 1].tolist()}")
            assert not info[:, 2].any() and not info[:, 3].any() and not info[:, 4].any(), info
            infos[(widen, fused)] = info
            if ref is None:
                ref = outs
            for k, (a, b) in enumerate(zip(ref, outs)):
                assert a[0] == b[0], f"H of factor {k} differs (widen {widen}, fused {fused})"
                assert a[1] == b[1], f"U of factor {k} differs (widen {widen}, fused {fused})"
            if not fused:
                assert count == 0
            elif widen:
                # one search launch per job and iteration run; a stopped job's blocks leave at
                # the stop test, so they publish nothing and never reach the second arrival
                assert count == int(info[:, 0].sum()), (count, info[:, 0])
    assert _lib.fault_repairs() == 0
    for key, info in infos.items():
        assert (info[:, :2] == infos[(0, True)][:, :2]).all(), key
    return infos[(0, True)]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def test_bits_equal_one_block_sweep(torch_dev):
    """Jobs of 1, a few and 9 blocks (partial last unit) and a layer4 shape, 6 iterations."""
    torch, dev = torch_dev
    info = _six_runs(torch, _problems(torch, dev, SHAPES, 1), 6, 0.0)
    assert (info[:, 1] == 0).all()   # eps = 0: nothing stops


def test_three_groups_per_thread(torch_dev):
    """Eight layer4 factors: more units than resident blocks at two float4 groups per thread,
    so the fused launch takes three (U re-read with H and F after the search)."""
    torch, dev = torch_dev
    _six_runs(torch, _problems(torch, dev, [(512, 1141)] * 8, 2), 3, 0.0)


def _ridge_problem(torch, dev, I, R, seed, ridge):
    """G = B B^T + ridge I, as tests/test_gpu_launch_head.py builds its early-exit problems."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((R, 2 * R)) / np.sqrt(2 * R)
    G = (B @ B.T + ridge * np.eye(R)).astype(np.float32)
    F = rng.standard_normal((I, R)).astype(np.float32)
    H = (rng.standard_normal((I, R)) * 0.1).astype(np.float32)
    return tuple(torch.from_numpy(a).to(dev) for a in (H, F, G))


def test_early_stop_mixed(torch_dev):
    """eps = 0.3 on the early-exit problems of tests/test_gpu_launch_head.py: the reference stops
    them at iterations 6, 8 and 13 (the stop test at least 12 % away from eps either side), so
    in a 10-iteration call two jobs stop while the third runs on. The stopped jobs' blocks
    leave at the stop test: the shared-stage-2 count is the sum of the iterations run."""
    torch, dev = torch_dev
    probs = [_ridge_problem(torch, dev, *spec) for spec in [(40, 70, 7, 4.0), (64, 134, 7, 0.5), (128, 183, 9, 0.08)]]
    info = _six_runs(torch, probs, 10, 0.3)
    assert info[:, 1].tolist() == [1, 1, 0], info   # two stopped, one running on
    assert info[0, 0] < info[1, 0] < info[2, 0], info


def test_thin_loop_window(torch_dev):
    """An all-thin call (I <= 16: the persistent thin loop, which has its own selection and
    stage 2): the knob's values 1 and 2 give the default run's bits there too."""
    torch, dev = torch_dev
    probs = _problems(torch, dev, [(9, 134), (9, 278)], 5)
    ref = None
    for widen in (0, 1, 2):
        outs, info, _ = _run(torch, probs, 6, 0.0, widen, True)
        assert not info[:, 2:].any(), info
        ref = ref or outs
        assert outs == ref, widen
