"""GPU checks of the Krylov block step's kernels (csrc/ortho_kernels.hip: admmq_cholqr64,
admmq_panel_reorth64) and of the fused route built on them (orthonormalize(fused=True),
KrylovProjector(fused=True), factorize_lowrank(projection="krylov-fused")), against float64
torch on the CPU. fp64 bounds are 1e-13, as in test_gpu_panel.py; the CPU float64 sCholQR3
gives 4e-16 to 1.6e-15 on the three orthonormalize measures for these inputs."""
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

DEV = "cuda:0"
SHAPES = [(33, 32), (70, 32), (257, 48), (300, 64), (65, 1), (130, 17)]


def _panel(m, k, ill=False):
    """randn(m, k), or with cond ~1e9..1e10: randn(m, k) diag(logspace(0, -8, k)) randn(k, k)."""
    g = torch.Generator().manual_seed(1000 * m + k)
    Z = torch.randn(m, k, generator=g, dtype=torch.float64)
    if ill:
        Z = (Z * torch.logspace(0, -8, k, dtype=torch.float64)) @ torch.randn(k, k, generator=g, dtype=torch.float64)
    return Z


def _decaying(m, n):
    """m x n float32 with singular values 2^-i."""
    g = torch.Generator().manual_seed(7)
    U = torch.linalg.qr(torch.randn(m, n, generator=g, dtype=torch.float64))[0]
    V = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))[0]
    return ((U * 2.0 ** -torch.arange(n, dtype=torch.float64)) @ V.T).float()


@pytest.mark.parametrize("shift_scale", [0.0, 1e-11])
@pytest.mark.parametrize("m,k,form", [(33, 32, "plain"), (70, 32, "strided"), (257, 48, "inplace"), (300, 64, "plain"),
                                      (65, 1, "plain"), (130, 17, "plain")])
def test_cholqr_one_pass(m, k, form, shift_scale):
    from admmq import panel
    Zc = _panel(m, k)
    Z = Zc.to(DEV)
    if form == "strided":   # ldz = k + 3 > k
        Z = torch.cat([Z, torch.zeros(m, 3, dtype=torch.float64, device=DEV)], 1)[:, :k]
    G = panel.gram(Z, Z)
    Q = panel.cholqr(Z, G, shift_scale, out=Z if form == "inplace" else None)
    assert (Q.data_ptr() == Z.data_ptr()) == (form == "inplace")
    Gc = G.cpu()
    L = torch.linalg.cholesky(Gc + shift_scale * torch.trace(Gc) * torch.eye(k, dtype=torch.float64))
    ref = torch.linalg.solve_triangular(L, Zc.T, upper=False).T
    err = float((Q.cpu() - ref).abs().max())
    print(f"cholqr {m}x{k} {form} shift {shift_scale}: max err {err:.2e}, max|Q| {float(ref.abs().max()):.2e}")
    assert err <= 1e-13 * float(ref.abs().max())


@pytest.mark.parametrize("ill", [False, True])
@pytest.mark.parametrize("m,k", SHAPES)
def test_orthonormalize_fused(m, k, ill):
    from admmq.lowrank import orthonormalize
    Zc = _panel(m, k, ill)
    Z = Zc.to(DEV)
    Q = orthonormalize(Z, fused=True).cpu()
    assert torch.equal(Z.cpu(), Zc)   # the caller's Z is not written
    R = Q.T @ Zc
    orth = float((Q.T @ Q - torch.eye(k, dtype=torch.float64)).abs().max())
    resid = float(torch.linalg.norm(Zc - Q @ R) / torch.linalg.norm(Zc))
    lower = float(torch.tril(R, -1).abs().max() / R.abs().max())
    print(f"orthonormalize {m}x{k} ill={ill}: orth {orth:.2e} resid {resid:.2e} lower {lower:.2e}")
    assert orth <= 1e-13 and resid <= 1e-13 and lower <= 1e-13


@pytest.mark.parametrize("with_info", [True, False])
def test_cholqr_not_positive_definite(with_info):
    from admmq import panel
    Z = _panel(70, 32).to(DEV)
    info = torch.zeros(1, dtype=torch.int32, device=DEV) if with_info else None
    Q = panel.cholqr(Z, -torch.eye(32, dtype=torch.float64, device=DEV), info=info)   # (raises unless ADMMQ_OK)
    assert bool(torch.isnan(Q).all())
    assert info is None or int(info[0]) == 1


@pytest.mark.parametrize("m,p,k", [(130, 96, 32), (70, 33, 17), (257, 192, 64), (64, 4, 1)])
def test_reorth(m, p, k):
    from admmq import panel
    g = torch.Generator().manual_seed(m + p + k)
    Kc, Cc, Zc = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((m, p), (p, k), (m, k)))
    K, C, Z = Kc.to(DEV), Cc.to(DEV), Zc.to(DEV)
    out = panel.reorth(K, C, Z)
    err = float((out.cpu() - (Zc - Kc @ Cc)).abs().max())
    bound = 1e-13 * float(Zc.abs().max() + p * Kc.abs().max() * Cc.abs().max())
    print(f"reorth {m}x{p}x{k}: max err {err:.2e}, bound {bound:.2e}")
    assert err <= bound
    assert torch.equal(out, panel.reorth(K, C, Z))   # the same bits on every call
    assert torch.equal(Z.cpu(), Zc)
    assert panel.reorth(K, C, Z, out=Z) is Z and torch.equal(Z, out)   # in place: the same bits


def test_projector_fused_matches_exact_truncation():
    from admmq.lowrank import KrylovProjector
    Xc = _decaying(256, 192)
    X = Xc.to(DEV)
    U, S, Vt = torch.linalg.svd(Xc.double(), full_matrices=False)
    for r, kw in ((8, {}), (48, {"block": 32})):
        exact = (U[:, :r] * S[:r]) @ Vt[:r]
        for fused in (True, False):
            P = KrylovProjector(r, fused=fused, **kw)
            got = P(X)
            rel = float(torch.linalg.norm(got.cpu().double() - exact) / torch.linalg.norm(exact))
            L, Rt = P.last_factors
            back = float(torch.linalg.norm(L @ Rt - got) / torch.linalg.norm(got))
            print(f"projector r={r} fused={fused}: rel {rel:.2e} blocks {P.blocks} repairs {P.repairs} factors {back:.2e}")
            assert rel <= 1e-4 and P.repairs == 0
            assert back <= 1e-5   # two float32 roundings of the factors and an r-term float32 sum


def test_outer_loop_krylov_fused():
    from admmq.lowrank import factorize_lowrank
    W = torch.randn(96, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    W_q, W_r, hist = factorize_lowrank(W, 4, 8, max_iter=2, inner_iter=5, projection="krylov-fused")
    assert len(hist) == 2 and bool(torch.isfinite(W_q).all()) and bool(torch.isfinite(W_r).all())
