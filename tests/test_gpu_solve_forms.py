"""Every form of the ADMM solve step H_T = P M (source/admm.py:56-57) held to a float64
reference element by element, at steps 1, 2 and 3 of a call.

Reference of step k + 1 for a problem (H0, U0, F, G): rho = float32(float32(trace64) / R) as
_fp64_ht of test_gpu_configs.py; P64 = F + rho (H_k + U_k) in float64 from the float32
values (H_0 = H0, U_0 = U0; H_k, U_k are what the same call returns with max_iter = k + 1:
calls are bit-reproducible); M is the device's own float32 inverse of A = G + rho I (the
float32 values the fill kernel forms, _lib.debug_spd_inverse), checked once per case to be
within 1e-7 relative Frobenius of numpy.linalg.inv(A) and zero outside R x R;
want = P64 M in float64.

Bound of the float32 forms (oracle/solve_bound.py has the derivation; nothing measured):

    |H_T[i,j] - want[i,j]| <= (R + 4) 2^-24 B[i,j],   B = (|F| + |rho| (|H_k| + |U_k|)) |M|

- R roundings of the dot product in any order (an MFMA K order, K-split piece sums, the thin
solve's chains), three forming P, one spare for the second-order terms.

Bound of solve="split" (fp16 hi/lo planes, gemm_kernels.hip k_gemm<.., SPLIT = true>). From
the code (quant_device.h split_store4, a row scaled by 2^e to max |x| 2^e in [2^14, 2^15)):
  * planes: hi = fp16(s), lo = fp16(s - hi) with s = x 2^e, both differences exact in
    float32, so |x - (hi + lo) 2^-e| <= 2^-22 |x| + 2^-25 2^-e (the second term where lo is
    an fp16 subnormal; 2^-e <= 2^-14 max|row|), for P and for M: 2 * 2^-22 = 8 u per product;
  * k_gemm multiplies Pl Mh, Ph Ml, Ph Mh and drops Pl Ml, |Pl Ml| <= 2^-22 |P| |M|: 4 u;
  * every fp16 x fp16 product is exact in float32; the epilogue's ldexp is exact.
What the code does not show is how v_mfma_f32_32x32x16_f16 rounds inside its 16-term sums
(3 R / 16 of them per element), so the accumulation term is measured, as the issue allows:
the worst |H_T - want| / B of the split form over this file's split cases and steps on the
MI355X is SPLIT_WORST below (7.03 2^-24, under the 12 u of the two derived terms alone), and
the test asserts 4 x that (the margin covers other seeds).
The thin factor of a split call takes the float32 VALU solve and is held to R + 4. The
1e-5 relative Frobenius check of the other files is kept beside it.

Each case prints its worst ratio err / (2^-24 B).
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

from conftest import gpu_available
from oracle import admm_oracle as ao
from oracle import solve_bound as sb

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MSE = sb.MSE
STEPS = 3
# worst |H_T - want| / B of solve="split" over SPLIT_SHAPES, steps 1..3, measured on the
# MI355X: 7.03 in units of 2^-24 = 4.19e-7, at (40, 357) step 2 ((65, 129): 5.64 at step 3;
# the fp32 tiles give 8.44 and 9.18 there), and the asserted multiple of it: 28.1 2^-24 B
SPLIT_WORST = 7.03 * 2.0 ** -24
SPLIT_FACTOR = 4.0
SPLIT_SHAPES = [(65, 129), (40, 357), (9, 134)]
KSPLIT = {(40, 357): 2, (70, 550): 3, (100, 745): 4}
_PROF_THIN_LOOP = 6   # include/admmq.h ADMMQ_PROF_THIN_LOOP


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(I, R):
    """The problem of a shape with its rho and the device's inverse, computed once and shared
    (read only). Asserts test_form0_is_the_inverse's rule for this M."""
    from admmq import _lib
    H0, U0, F, G = sb.solve_problem(I, R)
    rho = ao.rho_of(G)
    A = sb.device_a64(G, rho)
    (o,), _ = _lib.debug_spd_inverse([A], 0.0)
    M = o["M"]
    Mi = np.linalg.inv(A)
    assert o["flag"] == 0
    assert np.linalg.norm(M[:R, :R] - Mi) <= 1e-7 * np.linalg.norm(Mi), (I, R)
    assert not M[R:, :].any() and not M[:, R:].any(), (I, R)
    return dict(H0=H0, U0=U0, F=F, G=G, rho=rho, M=M[:R, :R].astype(np.float64))


def _banded(torch, dev, a, band):
    """`a` on the device as the middle of a flat buffer with `band` NaNs on both sides
    (band 64: 16-byte aligned; band 65: 4-byte aligned only). Returns (view, buffer)."""
    buf = torch.full((a.size + 2 * band,), float("nan"), dtype=torch.float32, device=dev)
    v = buf[band:band + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * band) % 16
    return v, buf


def _run_steps(torch_dev, shapes, solve=None, steps=STEPS, counts=None):
    """out[m - 2][k] = (H, U, H_T) in numpy of problem k after the call with max_iter = m, for
    m = 2 .. steps + 1, each on fresh copies of the inputs (eps = 0: nothing stops).
    `counts`: a list that receives every call's launch counts per class (admmq_profile_end)."""
    torch, dev = torch_dev
    from admmq import admm_iteration_batched, _lib
    lib = _lib.load()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = []
    for m in range(2, steps + 2):
        cs = [_case(I, R) for I, R in shapes]
        ps = [(t(c["H0"]), t(c["U0"]), t(c["F"]), t(c["G"])) for c in cs]
        ms, cnt = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)()
        if counts is not None:
            _lib.check(lib.admmq_profile_begin(256, 1), "profile_begin")
        try:
            Hs, dbg, info = admm_iteration_batched(ps, m, 0.0, 4, MSE, debug_outputs=True, return_info=True, solve=solve)
            torch.cuda.synchronize()
        finally:
            if counts is not None:
                _lib.check(lib.admmq_profile_end(ms, cnt), "profile_end")
                counts.append([int(c) for c in cnt])
        info = info.cpu().numpy()
        assert (info[:, 0] == m - 1).all() and (info[:, 1:] == 0).all(), info
        out.append([(H.cpu().numpy(), p[1].cpu().numpy(), d[0].cpu().numpy()) for H, p, d in zip(Hs, ps, dbg)])
    return out


def _check_steps(shapes, runs, label, limit=None):
    """Every problem's H_T of every step inside its bound; prints and returns the worst ratio
    err / (2^-24 B). `limit(I, R)`: the bound in units of 2^-24 B (default R + 4)."""
    worst = 0.0
    for k, (I, R) in enumerate(shapes):
        c = _case(I, R)
        Hk, Uk = c["H0"], c["U0"]
        lim = float(limit(I, R)) if limit else float(sb.fp32_constant(R))
        ratios = []
        for step, run in enumerate(runs):
            H, U, HT = run[k]
            assert HT.shape == (I, R)
            want, B = sb.reference(Hk, Uk, c["F"], c["rho"], c["M"])
            ratios.append(sb.worst_ratio(HT, want, B))
            Hk, Uk = H, U
        print(f"{label} ({I},{R}): worst err / (2^-24 B) at steps 1..{len(runs)}: "
              f"{' '.join('%.2f' % r for r in ratios)} (bound {lim:g})")
        for step, r in enumerate(ratios):
            assert r <= lim, (label, (I, R), step + 1, r, lim)
        worst = max(worst, max(ratios))
    return worst


@contextlib.contextmanager
def _setter(name, value, restore):
    """A debug setter of the library held for a block and restored after it."""
    from admmq import _lib
    fn = getattr(_lib.load(), name)
    args = lambda v: v if isinstance(v, tuple) else (v,)  # noqa: E731
    try:
        _lib.check(fn(*args(value)), name)
        yield
    finally:
        _lib.check(fn(*args(restore)), name)


def _same_runs(a, b):
    for ra, rb in zip(a, b):
        for x, y in zip(ra, rb):
            for u, v in zip(x, y):
                assert np.array_equal(_bits(u), _bits(v))


# ---------------------------------------------------------------------------- default kernel
@pytest.mark.parametrize("I,R", [(33, 33), (65, 129)], ids=lambda v: str(v))
def test_default_fp32_ragged(torch_dev, I, R):
    """(33, 33): one valid row in the second 32-row half of a 64-row tile and one column past
    a 32 block; (65, 129): two row tiles, three 32-column blocks (the last 64-column tile
    half full)."""
    from admmq import _lib
    assert _lib.load().admmq_debug_ksplit_pieces(I, R) == 1
    _check_steps([(I, R)], _run_steps(torch_dev, [(I, R)]), "fp32 default")


@pytest.mark.parametrize("form", [2, 0, 1], ids=["parallel", "serial", "launch"])
@pytest.mark.parametrize("I,R", list(KSPLIT), ids=lambda v: str(v))
def test_ksplit_pieces_alone(torch_dev, I, R, form):
    """A K-split factor alone in its launch, its pieces in parallel (np workgroups and the
    combine), folded serially, and as the launch chooses."""
    from admmq import _lib
    assert _lib.load().admmq_debug_ksplit_pieces(I, R) == KSPLIT[(I, R)]
    with _setter("admmq_debug_set_ksplit_form", form, 1):
        runs = _run_steps(torch_dev, [(I, R)])
    _check_steps([(I, R)], runs, f"fp32 K-split np={KSPLIT[(I, R)]} form {form}")


def test_ksplit_pieces_in_one_batch(torch_dev):
    """The three K-split factors in one batch with the serial fold, and as the launch chooses:
    inside the bound, and (pieces are fixed by the shape alone) the two equal bit for bit."""
    from admmq import _lib
    shapes = list(KSPLIT)
    for (I, R), np_ in KSPLIT.items():
        assert _lib.load().admmq_debug_ksplit_pieces(I, R) == np_
    with _setter("admmq_debug_set_ksplit_form", 0, 1):
        serial = _run_steps(torch_dev, shapes)
    _check_steps(shapes, serial, "fp32 K-split batch, serial")
    own = _run_steps(torch_dev, shapes)
    _check_steps(shapes, own, "fp32 K-split batch, launch's choice")
    _same_runs(serial, own)


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
def test_gemm_stage_forms(torch_dev, stage):
    with _setter("admmq_debug_set_gemm_stage", stage, 3):
        runs = _run_steps(torch_dev, [(65, 129)])
    _check_steps([(65, 129)], runs, f"fp32 gemm_stage {stage}")


def test_wide_tiles(torch_dev):
    """(130, 200) with the wide-tile threshold at zero: one 256 x 128 row tile, 130 valid rows,
    two column tiles (the second 72 columns of 128)."""
    from admmq import _lib
    assert _lib.load().admmq_debug_ksplit_pieces(130, 200) == 1   # a K-split factor never takes wide tiles
    with _setter("admmq_debug_set_wide_min_tiles", 0, 4 * 768):
        runs = _run_steps(torch_dev, [(130, 200)])
    _check_steps([(130, 200)], runs, "fp32 wide tiles")


# ------------------------------------------------------------------------------- split form
def _split_limit(I, R):
    return sb.fp32_constant(R) if I <= 16 else SPLIT_FACTOR * SPLIT_WORST / sb.U32


@pytest.mark.parametrize("I,R", SPLIT_SHAPES, ids=lambda v: str(v))
def test_split_form(torch_dev, I, R):
    runs = _run_steps(torch_dev, [(I, R)], solve="split")
    c = _case(I, R)
    want, _ = sb.reference(c["H0"], c["U0"], c["F"], c["rho"], c["M"])
    rel = sb.rel_frobenius(runs[0][0][2], want)
    print(f"split ({I},{R}): step 1 rel-Frobenius {rel:.2e}")
    assert rel < 1e-5
    _check_steps([(I, R)], runs, "split", _split_limit)


# ------------------------------------------------- persistent fp32 kernels, two-wave K-steps
def _tile_rows(rule, I, ld):
    """f32_tile_rows of admm_plan.hip."""
    if I <= 32:
        return 32
    big = ld >= 1024
    if rule == 0:
        return 64
    if rule == 2:
        return 64 if big else 32
    if rule == 3:
        return 128 if (big and I % 128 == 0) else 64
    return 128 if (big and I % 128 == 0) else 32


F32_SHAPES = [(20, 70), (65, 129), (128, 1000), (130, 1000)]


def _f32_id(kernel, rule):
    rows = ",".join(f"{I}x{R}:bm{_tile_rows(rule, I, (R + 31) // 32 * 32)}" for I, R in F32_SHAPES)
    return f"{'f32p' if kernel == 1 else 'f32t'}-rule{rule}[{rows}]"


F32_FORMS = [(k, r) for k in (1, 2) for r in (0, 1, 2, 3)]


@pytest.mark.parametrize("kernel,rule", F32_FORMS, ids=[_f32_id(k, r) for k, r in F32_FORMS])
def test_f32_persistent_kernels(torch_dev, kernel, rule):
    """k_gemm_f32p (kernel 1) and k_gemm_f32t (2) under every tile rule, one batch of
    (20, 70): 32-row factor; (65, 129): 32- or 64-row tiles by rule; (128, 1000): ld = 1024,
    128-row tiles under rules 1 and 3, 64 under 0 and 2; (130, 1000): never 128-row tiles.
    The case id names the tile rows f32_tile_rows gives each factor."""
    assert [_tile_rows(rule, 128, 1024), _tile_rows(rule, 130, 1024)] == [[64, 64], [128, 32], [64, 64], [128, 64]][rule]
    with _setter("admmq_debug_set_f32_persistent", (kernel, rule), (0, 1)):
        runs = _run_steps(torch_dev, F32_SHAPES)
    _check_steps(F32_SHAPES, runs, _f32_id(kernel, rule).split("[")[0])


@pytest.mark.parametrize("kernel", [1, 2], ids=["f32p", "f32t"])
def test_f32_persistent_32_row_statistics(torch_dev, kernel):
    """A 32-row tile of k_gemm_f32p / k_gemm_f32t has two sub-tile waves, the other tile shapes
    four, and the workgroup folds that many per-wave max|X| / min X / max X values into the
    quantizer's range. _check_steps cannot see that range (it takes H_k from the device), so:
    the (20, 70) factor sums the same two K-halves per element as the default kernel's 32-row
    tiles, hence its H, U and H_T of 3 steps equal the default run's bit for bit. (65, 129) is
    company in the launch only and is not compared (its rule-1 tiles are 32-row ones, which
    share f32p's workgroups; its bits differ from the default's 64-row tiles): r[0] below is
    the (20, 70) factor."""
    shapes = [(20, 70), (65, 129)]
    default = _run_steps(torch_dev, shapes)
    with _setter("admmq_debug_set_f32_persistent", (kernel, 1), (0, 1)):
        runs = _run_steps(torch_dev, shapes)
    _same_runs([[r[0]] for r in default], [[r[0]] for r in runs])


@pytest.mark.parametrize("I,R", [(65, 129), (64, 1000)], ids=lambda v: str(v))
def test_gemm_ks2(torch_dev, I, R):
    """Eight waves per 64 x 64 tile, two half chains per K-step summed in fixed order."""
    with _setter("admmq_debug_set_gemm_ks", 2, 1):
        runs = _run_steps(torch_dev, [(I, R)])
    _check_steps([(I, R)], runs, "fp32 gemm_ks 2")


# ------------------------------------------------------------------------------ thin factors
@pytest.mark.parametrize("rows", [(1, 9), (10, 16)], ids=["thin_solve9", "thin_solve16"])
@pytest.mark.parametrize("R", [33, 134, 1152, 1185, 2400])
def test_thin_per_iteration(torch_dev, R, rows):
    """k_thin_solve<9> (largest thin I <= 9) and <16>, per-iteration launches, beside a
    (40, 70) factor: R = 33, 134 one reduction chunk, 1152 exactly one, 1185 two (the second
    a single 64-wide piece), 2400 three."""
    from admmq import _lib
    shapes = [(I, R) for I in rows] + [(40, 70)]
    with _lib.thin_loop(False):
        runs = _run_steps(torch_dev, shapes)
    _check_steps(shapes, runs, f"thin per-iteration {rows}")


@pytest.mark.parametrize("width", [True, "wide"], ids=["default", "wide"])
def test_thin_loop(torch_dev, width):
    """The persistent thin loop on an all-thin batch (one ld = 512 factor), 32-column teams
    and 64-column ones: the loop ran (its launch class counts one launch per call, no
    per-iteration launch) and every step is inside the bound."""
    from admmq import _lib
    shapes = [(9, 134), (16, 40), (1, 33), (12, 500)]
    counts = []
    with _lib.thin_loop(width):
        runs = _run_steps(torch_dev, shapes, counts=counts)
    print("launches per class, max_iter 2..4:", counts)
    for m, got in zip(range(2, STEPS + 2), counts):
        if m > 2:   # the calls with more than one iteration: one loop launch, no per-iteration launch
            assert got[_PROF_THIN_LOOP] == 1 and got[0] == got[1] == got[2] == got[3] == got[4] == 0, (m, got)
        assert got[7] == 0, (m, got)
    _check_steps(shapes, runs, f"thin loop {width}")


# ------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("I,R", [(65, 129), (9, 134)], ids=lambda v: str(v))
def test_guard_bands(torch_dev, I, R):
    """H0, U, F and G as views inside NaN-filled buffers, 16-byte aligned (band 64) and
    4-byte aligned only (band 65): H, U and H_T of 3 iterations equal the plain run's bit for
    bit, every band and every input but U keeps its bits."""
    torch, dev = torch_dev
    from admmq import admm_iteration_batched
    c = _case(I, R)
    plain = _run_steps(torch_dev, [(I, R)])[-1][0]
    for band in (64, 65):
        views, bufs = zip(*[_banded(torch, dev, c[k], band) for k in ("H0", "U0", "F", "G")])
        before = [b.clone() for b in bufs]
        (H,), dbg = admm_iteration_batched([tuple(views)], STEPS + 1, 0.0, 4, MSE, debug_outputs=True)
        got = (H.cpu().numpy(), views[1].cpu().numpy(), dbg[0][0].cpu().numpy())
        for a, b in zip(got, plain):
            assert np.array_equal(_bits(a), _bits(b)), band
        for k, (b, b0) in enumerate(zip(bufs, before)):
            b, b0 = b.view(torch.int32), b0.view(torch.int32)
            if k == 1:   # U: the interior is the output, the bands stay
                assert torch.equal(b[:band], b0[:band]) and torch.equal(b[-band:], b0[-band:]), band
            else:
                assert torch.equal(b, b0), (band, k)
