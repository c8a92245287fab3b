"""The forms of the SPD inverse M = (G + rho I)^-1 (csrc/spd_kernels.hip, DESIGN.md §8.5;
admmq_debug_set_spd_form): bit 0 the one-launch Cholesky block column (k_chol_step), bit 1 the
wide L^-1 column slices (k_linv_cols_w, 8 or 16 columns), bit 2 the register-tile k_minv.

Every form keeps each element's chain of fp64 operations, so against form 0 (the earlier
kernels) the inverse itself is compared bit for bit, read out by admmq_debug_spd_inverse:
M, the diagonal L blocks (D64), L in the strictly lower blocks of A64 and L^-1 in the lower
blocks of L64. Then the callers: the blocked EPC step and a batched ADMM call."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE = "tensor_mseminmax_symmetric"
# R = 20: one block (no off-diagonal work, no column kernel); 33: two blocks (the first fused
# update, no trailing workgroup); 70: three blocks, ragged (the first trailing workgroup);
# 278: nine blocks (a column-kernel group owns a second pending S); the batch: problems that
# go idle in later launches, maxnbk != own nbk
CASES = {"R20": [20], "R33": [33], "R70": [70], "R278": [278], "batch": [20, 70, 134, 278]}
# (mask, slice width): every bit alone and all together; the wide slices at both widths and
# at the launcher's own choice
FORMS = [(1, 0), (2, 8), (2, 16), (2, 0), (4, 0), (7, 8), (7, 16), (7, 0)]


def _spd(R, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((R, 2 * R)) / np.sqrt(2 * R)
    return B @ B.T + 0.05 * np.eye(R)


def _run(Gs, mask, width=0, shift=0.25):
    from admmq import _lib
    with _lib.spd_form(mask, width):
        return _lib.debug_spd_inverse(Gs, shift)[0]


def _lower_blocks(a, strict):
    """The 32 x 32 blocks (i, j), j < i (or j <= i), of a square matrix, as one array."""
    n = a.shape[0] // 32
    return np.stack([a[32 * i:32 * i + 32, 32 * j:32 * j + 32] for i in range(n) for j in range(i + (0 if strict else 1))]
                    or [np.zeros((32, 32), a.dtype)])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_same(got, ref, what):
    assert got["flag"] == ref["flag"], what
    assert _same_bits(got["M"], ref["M"]), (what, "M")
    assert _same_bits(got["D"], ref["D"]), (what, "D64")
    assert _same_bits(_lower_blocks(got["A"], True), _lower_blocks(ref["A"], True)), (what, "L")
    assert _same_bits(_lower_blocks(got["Linv"], False), _lower_blocks(ref["Linv"], False)), (what, "Linv")


_REF = {}


def _case(name):
    """The case's matrices and their inverse under form 0, computed once."""
    if name not in _REF:
        Gs = [_spd(R, 100 + R) for R in CASES[name]]
        _REF[name] = (Gs, _run(Gs, 0))
    return _REF[name]


@pytest.mark.parametrize("case", list(CASES))
def test_form0_is_the_inverse(case):
    """Form 0 itself against the fp64 library inverse (the reference every form is held to):
    M is fp64 work (condition number ~10, error ~1e-15) rounded once to fp32, 2^-24 = 6e-8
    relative per element, so 1e-7 in the Frobenius norm; zero outside R x R."""
    Gs, ref = _case(case)
    for G, o in zip(Gs, ref):
        R = G.shape[0]
        Mi = np.linalg.inv(G + 0.25 * np.eye(R))
        assert o["flag"] == 0
        assert np.linalg.norm(o["M"][:R, :R] - Mi) <= 1e-7 * np.linalg.norm(Mi)
        assert not o["M"][R:, :].any() and not o["M"][:, R:].any()


@pytest.mark.parametrize("mask,width", FORMS)
@pytest.mark.parametrize("case", list(CASES))
def test_forms_bit_equal_form0(case, mask, width):
    Gs, ref = _case(case)
    got = _run(Gs, mask, width)
    for R, g, r in zip(CASES[case], got, ref):
        _assert_same(g, r, (case, R, mask, width))


def test_default_form_twice_and_its_bits():
    """The default form on the batch: two runs give the same bits, and they are form 0's."""
    from admmq import _lib
    Gs, ref = _case("batch")
    a, b = _run(Gs, None), _run(Gs, None)
    for R, x, y, r in zip(CASES["batch"], a, b, ref):
        _assert_same(x, y, (R, "rerun"))
        _assert_same(x, r, (R, "default", _lib.load().admmq_debug_get_spd_form_default()))


def test_largest_benchmark_rank():
    """R = 1141 (36 blocks), the benchmark's largest: every new form at once, at the launcher's
    own slice width, against form 0."""
    G = _spd(1141, 7)
    ref = _run([G], 0)[0]
    _assert_same(_run([G], 7)[0], ref, 1141)


def test_non_spd_sets_the_flag_and_spares_the_batch():
    """A G with one negative eigenvalue (R = 70, deterministic) between two SPD problems:
    flags[2] is set for it in both forms, the call returns, and the other problems keep the
    bits they have without it."""
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.standard_normal((70, 70)))
    lam = np.linspace(0.5, 2.0, 70)
    lam[17] = -1.0
    bad = (Q * lam) @ Q.T
    bad = 0.5 * (bad + bad.T)
    good = [_spd(70, 1), _spd(134, 2)]
    alone = _run(good, 0)
    for mask in (0, 7):
        out = _run([good[0], bad, good[1]], mask)
        assert [o["flag"] for o in out] == [0, 1, 0], mask
        _assert_same(out[0], alone[0], (mask, 70))
        _assert_same(out[2], alone[1], (mask, 134))


def test_blocked_epc_step_same_bits():
    """One blocked EPC step (solve64.hip, n = 200: a Cholesky and L^-1 per evaluation through
    launch_spd_linv, and the rounds after the search is done, whose descriptor has nbk = 0)
    under form 0 and the default: X and mu bit-equal."""
    import torch
    from admmq import _lib, panel
    g = torch.Generator().manual_seed(200)
    B = torch.randn(200, 208, generator=g, dtype=torch.float64)
    G = B @ B.T / 208 + 1e-3 * torch.eye(200, dtype=torch.float64)
    F = torch.randn(16, 200, generator=g, dtype=torch.float64)
    ls = float(torch.sum(F * torch.linalg.solve(G, F.T).T))
    normY2 = ls * 1.5
    delta2 = (normY2 - ls) * 1.5
    res = []
    for mask in (0, None):
        with _lib.spd_form(mask):
            mu = torch.zeros((), dtype=torch.float64, device="cuda")
            info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
            X = panel.epc_step64(G.cuda(), F.cuda(), normY2, delta2, mu, info=info)
            # the search is done: another round on the same inputs starts from its mu
            X2 = panel.epc_step64(G.cuda(), F.cuda(), normY2, delta2, mu, info=info)
            assert int(info) == 0
            res.append((X.cpu().numpy(), X2.cpu().numpy(), float(mu)))
    assert res[0][2] > 0.0 and res[0][2] == res[1][2]
    assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1])


def test_admm_batched_same_bits():
    """admm_iteration_batched, 6 iterations, on the four-layer batch of
    test_batched_equals_single_and_deterministic, under form 0 and the default: H and U."""
    import torch
    from admmq import _lib, admm_iteration_batched, synthetic
    from oracle import admm_oracle as ao
    dev = torch.device("cuda:0")
    probs = []
    for layer, mode in [("layer1.0.conv1", 2), ("layer2.1.conv1", 0), ("layer4.1.conv2", 1), ("layer3.0.conv1", 2)]:
        idx, spec = synthetic.find_layer("resnet18", layer)
        W = synthetic.layer_weight(spec, idx)
        gen = torch.Generator().manual_seed(42)
        fs = [torch.randn(n, spec.rank(), generator=gen).numpy() for n in W.shape]
        G, F = ao.gram_mttkrp(W, fs, mode)
        probs.append((fs[mode], F, G))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731

    def run(mask):
        with _lib.spd_form(mask):
            ps = [(t(H), torch.zeros(H.shape, device=dev), t(F), t(G)) for H, F, G in probs]
            Hs = admm_iteration_batched(ps, 6, 0.0, 4, MSE)
            return [(H.cpu().numpy(), p[1].cpu().numpy()) for p, H in zip(ps, Hs)]

    for (h0, u0), (h1, u1) in zip(run(0), run(None)):
        assert _same_bits(h0, h1) and _same_bits(u0, u1)
