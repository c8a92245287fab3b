"""Skinny integer quant + low-rank GEMV on the MI355X: k_ilr_down_gemv + k_packed_ilrgemv
(+ k_packed_ilrgemv_reduce) against the float64 numpy restatement of the contract in include/admmq.h (factors rounded
to T, t left in float64) - exact where every intermediate is representable, packed_linear_int's bits with L = 0 at
every width, the derived bound on random data, rows alone, guards, both binding routes and the layer's flag."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import gpu_available
from test_gpu_packed_hgemm import AFF, DEV, DTYPES, MSE, SYM, _packed, _randn
from test_gpu_packed_ilrgemm import _codes, _ref, _xq

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

# (M, K, r) -> (ns > 1, nsd) of admmq_packed_ilrgemv_plan at every width: what each shape is here for
PLANS = {(33, 65, 5): (False, 1),      # two row tiles, the second with one live row; one partial chunk; r % 4 != 0
         (65, 261, 37): (False, 2),    # nsd = 2 with a last range of 5 k; two tail steps, the second partial
         (33, 4100, 9): (True, 9),     # the K split of the code sum: the tail slice and the reduce
         (1, 7, 1): (False, 1),        # the degenerate case
         (33, 65, 256): (False, 1)}    # the full t image at N = 8
ROWS = [1, 2, 3, 8]                    # the four NB instantiations; 3 leaves a zero column
BITS_SCHEMES = [(3, AFF), (4, MSE), (8, SYM)]
XQ_EXACT = (2, -0.5, 0.75)             # g = 0.25
XQ8 = (8, -1.3, 2.9)
OUT_ACT = (4, -2.0, 2.0)


def _run(p, L, Rt, xq, bias=None, act=None, out_codes=False, T=torch.bfloat16, skinny=True):
    from admmq import PackedLowRank, packed_lowrank_linear_int
    return packed_lowrank_linear_int(xq, PackedLowRank(q=p, L=L, Rt=Rt), bias, act, out_codes, T, skinny=skinny)


def test_the_shapes_run_the_plans_they_are_named_for():
    from admmq import _lib
    from test_packed_hgemm_host import _meta
    for (M, K, r), (split, nsd) in PLANS.items():
        for bits in range(1, 9):
            out = (ctypes.c_int32 * 4)()
            assert _lib.load().admmq_packed_ilrgemv_plan(ctypes.byref(_meta(bits=bits)), M, K, r, out) == 0
            assert (out[1] > 1, out[2], out[3]) == (split, nsd, 3 if split else 2), (M, K, r, bits, tuple(out))


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("shape", list(PLANS))
def test_exact_where_every_intermediate_is_representable(shape, N, T):
    """L, Rt in {-1, 0, 1} (Rt half zeros), 2-bit codes with g = 0.25, mn_x = -0.5, integer biases: U32, t32 (a multiple
    of 0.25 below 2^24 / 4) and q are exact, so y is the float64 formula rounded once. No tolerance."""
    M, K, r = shape
    g = torch.Generator().manual_seed(3)
    L = torch.randint(-1, 2, (M, r), generator=g).float().to(DEV)
    Rt = (torch.randint(-1, 2, (r, K), generator=g) * torch.randint(0, 2, (r, K), generator=g)).float().to(DEV)
    bias = torch.randint(-9, 10, (M,), generator=g).float().to(DEV)
    xq = _xq(_codes((N, K), 2, 4), XQ_EXACT)
    for bits, scheme in BITS_SCHEMES:
        p, D = _packed((M, K), bits, scheme)
        want, t = _ref(p, D, L, Rt, xq, bias, T, round_t=False)
        assert (t.astype(np.float32).astype(np.float64) == t).all() and np.abs(t).max() * r < 2 ** 22   # a condition on the inputs
        want = torch.from_numpy(want.astype(np.float32)).to(DEV)
        for fl, fr in [(L, Rt), (L.to(T), Rt.to(T))]:
            assert torch.equal(_run(p, fl, fr, xq, bias, T=T), want), (bits, scheme, fl.dtype)


@pytest.mark.parametrize("scheme", [MSE, SYM, AFF])
@pytest.mark.parametrize("bits", range(1, 9))
@pytest.mark.parametrize("shape", [(33, 65, 5), (33, 4100, 9)])
def test_a_zero_L_gives_packed_linear_int(shape, bits, scheme):
    """q is an exact +0: all three output forms and the counter, both plans, with a bias and without, against the
    default integer route and its skinny one (torch.equal: -0 == +0)."""
    from admmq import packed_linear_int
    from test_gpu_packed_igemm import _weight   # (8-bit affine: a range whose zero_point stays inside int8)
    M, K, r = shape
    L, Rt, bias = torch.zeros(M, r, device=DEV), _randn((r, K), 17, 0.5), _randn((M,), 16)
    xq = _xq(_codes((8, K), 8, 5), XQ8)
    p = _weight((M, K), bits, scheme)[0]
    for b in (bias, None):
        for sk in (False, True):
            assert torch.equal(_run(p, L, Rt, xq, b), packed_linear_int(xq, p, b, skinny=sk))
            assert torch.equal(_run(p, L, Rt, xq, b, OUT_ACT), packed_linear_int(xq, p, b, act=OUT_ACT, skinny=sk))
            got, want = _run(p, L, Rt, xq, b, OUT_ACT, True), packed_linear_int(xq, p, b, act=OUT_ACT, out_codes=True, skinny=sk)
            assert torch.equal(got.codes, want.codes) and int(got.clamped) == int(want.clamped)


RATIOS = []


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("shape", list(PLANS))
def test_bound_against_float64(shape, N, T):
    """|y - y64| <= gamma B + eps |y64| elementwise, gamma = (1 + eps)^(K + r + 15) - 1, eps = 2^-24 (float32's unit
    roundoff), B = |L_T| (|Rt_T| (g ux + |mn_x|)), y64 on the factors as rounded to T with t unrounded: no u term
    (DESIGN.md 2.38 counts the 15). Derived, not tuned. Float32 factors and the same factors in T give the same bits.
    Largest ratio measured on the MI355X over all cases: 0.10."""
    M, K, r = shape
    eps = 2.0 ** -24
    gam = (1.0 + eps) ** (K + r + 15) - 1.0
    L, Rt, bias = _randn((M, r), 5 + M + r, 0.5).to(T), _randn((r, K), 6 + K + r, 0.5).to(T), _randn((M,), 12)
    xq = _xq(_codes((N, K), 8, 11 + N), XQ8)
    xabs = xq.codes.cpu().numpy().astype(np.float64) * (np.float64(np.float32(xq.rng)) / 255) + abs(xq.mn)
    B = (xabs @ np.abs(Rt.double().cpu().numpy()).T) @ np.abs(L.double().cpu().numpy()).T
    for bits, scheme in BITS_SCHEMES:
        p, D = _packed((M, K), bits, scheme)
        y = _run(p, L.float(), Rt.float(), xq, bias, T=T)
        assert torch.equal(y, _run(p, L, Rt, xq, bias, T=T)), (bits, scheme)
        y64 = _ref(p, D, L, Rt, xq, bias, T, round_t=False)[0]
        err, bound = np.abs(y.double().cpu().numpy() - y64), gam * B + eps * np.abs(y64)
        RATIOS.append(float((err / np.maximum(bound, 1e-300)).max()))
        print(f"{shape} N {N} {T} w bits {bits} {scheme}: max |err| / bound = {RATIOS[-1]:.4f} (largest so far {max(RATIOS):.4f})")
        assert tuple(y.shape) == (N, M) and bool((err <= bound).all())


@pytest.mark.parametrize("shape", [(65, 261, 37), (33, 4100, 9)])
def test_rows_alone_repeats_canaries_and_an_odd_address(shape):
    """Row c of an 8-row call against the 1-row call on that row and a repeated call; then canaries round y / y_codes
    and behind the stated workspace bytes with ux one byte past a 16-byte boundary and factors in T, through ctypes."""
    from admmq import _lib, packed_lowrank_factorsums, packed_rowsums, PackedLowRank
    from admmq.packed import HALF_DTYPES, _meta_words
    (M, K, r), N, T = shape, 8, torch.bfloat16
    p = _packed((M, K), 4, MSE)[0]
    L, Rt, bias = _randn((M, r), 21, 0.5), _randn((r, K), 22, 0.5), _randn((M,), 23)
    xq = _xq(_codes((N, K), 8, 24), XQ8)
    y = _run(p, L, Rt, xq, bias, T=T)
    assert torch.equal(y, _run(p, L, Rt, xq, bias, T=T))
    for c in (0, 5, 7):
        assert torch.equal(_run(p, L, Rt, _xq(xq.codes[c:c + 1].clone(), XQ8), bias, T=T)[0], y[c]), c
    lib, LT, RT = _lib.load(), L.to(T).contiguous(), Rt.to(T).contiguous()
    rho, rs = packed_lowrank_factorsums(PackedLowRank(q=p, L=LT, Rt=RT), T), packed_rowsums(p)
    meta = _lib.QMeta.from_buffer_copy(_meta_words(p).numpy().tobytes())
    need = lib.admmq_packed_ilrgemv_workspace_size(ctypes.byref(meta), M, K, N, r)
    xbuf = torch.zeros(N * K + 32, dtype=torch.uint8, device=DEV)
    xbuf[17:17 + N * K] = xq.codes.reshape(-1)
    xr, oq = _lib.ActQ(8, 1, xq.mn, xq.rng), _lib.ActQ(4, 1, -2.0, 4.0)
    for out_codes in (False, True):
        ybuf = torch.full((N * M + 64,), 7 if out_codes else -77.0, dtype=torch.uint8 if out_codes else torch.float32, device=DEV)
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        cl = torch.full((3,), -5, dtype=torch.int32, device=DEV)
        yp = ybuf[32:32 + N * M]
        rc = lib.admmq_packed_ilrgemv(_lib.ptr(p.codes), ctypes.byref(meta), M, K, _lib.ptr(LT), _lib.ptr(RT), HALF_DTYPES[T],
                                      HALF_DTYPES[T], r, _lib.ptr(rho), _lib.ptr(xbuf[17:]), ctypes.byref(xr), _lib.ptr(rs), N,
                                      _lib.ptr(bias), None if out_codes else _lib.ptr(yp), _lib.ptr(yp) if out_codes else None,
                                      ctypes.byref(oq) if out_codes else None, _lib.ptr(cl[1:]) if out_codes else None,
                                      _lib.ptr(ws), need, _lib.stream_handle(DEV))
        assert rc == 0, lib.admmq_last_error()
        want = _run(p, L, Rt, xq, bias, OUT_ACT, True, T) if out_codes else y
        assert torch.equal(yp.view(N, M), want.codes if out_codes else want)
        pad = 7 if out_codes else -77.0
        assert bool((ybuf[:32] == pad).all()) and bool((ybuf[32 + N * M:] == pad).all()) and bool((ws[need:] == 0xA5).all())
        if out_codes:
            assert cl.tolist() == [-5, int(want.clamped), -5]


def test_bindings_the_layer_flag_and_state(monkeypatch):
    """ops route == ctypes route; IntegerPackedLowRank.skinny sends 8 rows to the new route and leaves 9 rows on the
    default one; a state dict saved before the flag loads unchanged."""
    import admmq
    from admmq import _lib, export
    M, K, r = 33, 65, 5
    p = _packed((M, K), 4, SYM)[0]
    pl = admmq.PackedLowRank(q=p, L=_randn((M, r), 41, 0.5), Rt=_randn((r, K), 42, 0.5))
    bias, x8, x9, act = _randn((M,), 43), _randn((2, 4, K), 44, 0.4), _randn((9, K), 45, 0.4), (8, -2.0, 2.0)
    xq = admmq.act_encode(x8, act, check=False)
    y = admmq.packed_lowrank_linear_int(xq, pl, bias, skinny=True)
    direct = admmq.packed_ilrgemv(p.codes, admmq.packed._meta_words(p), M, K, pl.L, pl.Rt, admmq.packed_lowrank_factorsums(pl),
                                  xq, admmq.packed_rowsums(p), bias)
    assert tuple(y.shape) == (2, 4, M) and torch.equal(direct, y)
    assert not torch.equal(y, admmq.packed_lowrank_linear_int(xq, pl, bias))   # t is not rounded to T: other bits
    monkeypatch.setattr(_lib, "use_ops", lambda: False)
    assert torch.equal(admmq.packed_lowrank_linear_int(xq, admmq.PackedLowRank(q=p, L=pl.L, Rt=pl.Rt), bias, skinny=True), y)
    monkeypatch.undo()
    lay = export.build_qlr_layer(pl, bias, integer=True, in_act=act)
    old_state, plain8, plain9 = lay.state_dict(), lay(x8), lay(x9)
    lay.skinny = True
    assert torch.equal(lay(x8), y) and not torch.equal(plain8, y) and torch.equal(lay(x9), plain9)
    assert "skinny=True" in lay.extra_repr() and lay.state_dict().keys() == old_state.keys()
    lay.load_state_dict(old_state)
    assert lay.skinny and torch.equal(lay(x8), y)
