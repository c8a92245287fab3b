"""The quant + low-rank route's deployable ending: factorize_lowrank(..., return_packed=True)
returns W_q as packed codes that decode to it bit for bit and W_r as the thin pair the last rank
projection multiplied out, the default returns are unchanged by it, build_qlr_layer runs the result
within the fused GEMM's forward bound, and the CLI's --save-packed file loads into that layer."""
import functools
import glob
import os

import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

DEV = torch.device("cuda:0")
U = 2.0 ** -24
BITS, RANK = 4, 4


def _weight():
    g = torch.Generator().manual_seed(1234)
    return (torch.randn(96, 80, generator=g) * 0.05).to(DEV)


@functools.lru_cache(maxsize=None)
def _run(projection, qscheme, packed):
    """One seeded run - computed once, never modified."""
    from admmq.lowrank import factorize_lowrank
    return factorize_lowrank(_weight(), bits=BITS, rank=RANK, qscheme=qscheme, max_iter=3, inner_iter=6,
                             projection=projection, return_packed=packed)


def _forward_bound(y, D, L, Rt, x, what):
    """|y - y64| <= (K + r + 4) 2^-24 (|D||x| + |L|(|Rt||x|)) elementwise in float64 (test_gpu_packed_lrgemm.py)."""
    K, r = D.shape[1], L.shape[1]
    D64, L64, R64, x64 = D.double().cpu(), L.double().cpu(), Rt.double().cpu(), x.double().cpu()
    y64 = x64 @ (D64 + L64 @ R64).T
    mag = x64.abs() @ D64.abs().T + (x64.abs() @ R64.abs().T) @ L64.abs().T
    err = (y.double().cpu() - y64).abs()
    bound = (K + r + 4) * U * mag
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |err| / bound = {ratio:.4f}")
    assert bool((err <= bound).all()), f"{what}: max |err| / bound = {ratio}"


@pytest.mark.parametrize("qscheme", ["tensor_minmax", "tensor_mseminmax_symmetric"])
@pytest.mark.parametrize("projection", ["krylov", "svd"])
def test_return_packed(projection, qscheme):
    from admmq import PackedLowRank, export
    W_q, W_r, hist, packed = _run(projection, qscheme, True)
    assert isinstance(packed, PackedLowRank) and packed.rank == RANK
    assert tuple(packed.q.shape) == (96, 80) and packed.q.bits == BITS and packed.q.qscheme == qscheme
    assert tuple(packed.L.shape) == (96, RANK) and tuple(packed.Rt.shape) == (RANK, 80)
    assert packed.L.dtype == packed.Rt.dtype == torch.float32 and packed.Rt.is_contiguous() and packed.L.is_contiguous()
    # W_q's codes decode to it bit for bit
    assert torch.equal(packed.q.dequantize(), W_q)
    # the pair multiplies out to W_r: two factor roundings, W_r's own, the float32 r-term product of "svd"
    L64, R64 = packed.L.double().cpu(), packed.Rt.double().cpu()
    err = (L64 @ R64 - W_r.double().cpu()).abs()
    bound = (RANK + 4) * U * (L64.abs() @ R64.abs())
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{projection} {qscheme}: |L Rt - W_r| max / bound = {ratio:.4f}")
    assert bool((err <= bound).all()), ratio
    # the default returns are what they were
    plain = _run(projection, qscheme, False)
    assert len(plain) == 3
    assert torch.equal(plain[0], W_q) and torch.equal(plain[1], W_r) and plain[2] == hist
    # the layer runs the result
    g = torch.Generator().manual_seed(5)
    x = torch.randn(7, 80, generator=g).to(DEV)
    lin = export.build_qlr_layer(packed)
    _forward_bound(lin(x), W_q, packed.L, packed.Rt, x, f"layer {projection} {qscheme}")
    assert packed.nbytes == 96 * 80 // 2 + 4 * RANK * (96 + 80)


def test_a_run_without_a_quantizing_projection_has_no_grid():
    from admmq.lowrank import factorize_lowrank
    with pytest.raises(RuntimeError, match="no quantizing projection"):
        factorize_lowrank(_weight(), bits=BITS, rank=RANK, max_iter=1, inner_iter=1, projection="svd", return_packed=True)


def test_cli_save_packed_builds_the_layer(tmp_path):
    """python -m admmq.lowrank --save-packed -> load_packed_lowrank -> build_qlr_layer -> forward."""
    import admmq
    from admmq import export, lowrank
    layer = "blocks.0.proj"
    wpath = str(tmp_path / "weights.pt")
    torch.save({f"{layer}.weight": _weight().cpu()}, wpath)
    out = str(tmp_path / "out")
    W_q, W_r, hist = lowrank.main(["--max-iter", "2", "--bits", str(BITS), "--rank", str(RANK), "--layer", layer,
                                   "--weights", wpath, "--output-dir", out, "--projection", "svd", "--save-packed"])
    files = sorted(os.path.basename(f) for f in glob.glob(os.path.join(out, "*")))
    stem = f"{layer}_{BITS}_{RANK}_{hist[-1]:.3f}"
    assert files == [f"{stem}_Q.pt", f"{stem}_QR_packed.pt", f"{stem}_R.pt"]
    p = admmq.load_packed_lowrank(os.path.join(out, f"{stem}_QR_packed.pt"), device=DEV)
    assert torch.equal(p.q.dequantize(), W_q) and p.rank == RANK
    assert torch.equal(torch.load(os.path.join(out, f"{stem}_Q.pt"), weights_only=True), W_q.cpu())
    lin = export.build_qlr_layer(p)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, 80, generator=g).to(DEV)
    _forward_bound(lin(x), W_q, p.L, p.Rt, x, "cli layer")
