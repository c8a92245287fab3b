"""CPU test of the fused Cholesky launch's workgroup map (csrc/spd_kernels.hip k_chol_step,
chol_step_work; read out through admmq_debug_chol_step_work, host code only).

Launch s holds, per problem, the column workgroups (i, s), i >= s, and for s > 0 the trailing
workgroups (i, j), s < j <= i. What each of them touches in A64 (32 x 32 blocks):

  column (i, s), s > 0   applies update s - 1 to its own block (i, s) (and, in LDS only, to
                         A_ss); reads (s, s - 1), (i, s - 1), (s, s), (i, s)
  column (i, s)          factors: writes L_is to (i, s) for i > s; L_ss goes to D64 and the
                         diagonal block of A64 is not written
  trailing (i, j)        applies update s - 1 to (i, j); reads (i, s - 1), (j, s - 1), (i, j)

Checked for single problems and mixed batches: every block takes updates 0 .. j - 1 once each
in ascending order and is factored after the last of them, no block is written by two
workgroups of one launch, and no block is read in a launch in which another workgroup writes
it."""
import pytest

BATCHES = [[1], [2], [3], [9], [36], [1, 3, 5, 9], [9, 2, 36, 1, 3], [3, 3]]


def _simulate(nbk):
    from admmq import _lib
    maxnbk = max(nbk)
    updates = {(p, i, j): [] for p, n in enumerate(nbk) for i in range(n) for j in range(i + 1)}
    factored = {}
    for s in range(maxnbk):
        work, nwg = _lib.chol_step_work(s, nbk)
        n = maxnbk - s - 1
        assert nwg == len(nbk) * ((maxnbk - s) + (n * (n + 1) // 2 if s > 0 else 0))
        # every block a problem has in this launch appears, nothing else does
        expect = {(p, i, s) for p, b in enumerate(nbk) for i in range(s, b)}
        if s > 0:
            expect |= {(p, i, j) for p, b in enumerate(nbk) for i in range(s + 1, b) for j in range(s + 1, i + 1)}
        assert len(work) == len(set(work)) and set(work) == expect, (nbk, s)
        writes, reads = {}, []
        for w, (p, i, j) in enumerate(work):
            assert s <= j <= i < nbk[p]
            blk = (p, i, j)
            if s > 0:
                assert not (blk in factored), (blk, s)
                updates[blk].append(s - 1)
            if j == s:
                assert updates[blk] == list(range(j)), (blk, updates[blk])   # all of them, before the factorisation
                factored[blk] = s
                rd = [(p, s, s), blk] + ([(p, s, s - 1), (p, i, s - 1)] if s > 0 else [])
                wr = [blk] if i > s else []          # L_ss goes to D64
            else:
                rd = [(p, i, s - 1), (p, j, s - 1), blk]
                wr = [blk]
            for b in wr:
                assert b not in writes, (nbk, s, b)   # one writer per block and launch
                writes[b] = w
            reads += [(b, w) for b in rd]
        for b, w in reads:
            assert writes.get(b, w) == w, (nbk, s, b)  # read only by the workgroup that writes it
        for (p, i, k) in [b for b, _ in reads if b[2] == s - 1]:
            assert factored.get((p, i, k)) == s - 1    # column s - 1 was finished by the launch before
    assert set(factored) == set(updates)
    for (p, i, j), u in updates.items():
        assert u == list(range(j)) and factored[(p, i, j)] == j


@pytest.mark.parametrize("nbk", BATCHES, ids=lambda b: "-".join(map(str, b)))
def test_chol_step_map(nbk):
    _simulate(nbk)


def test_chol_step_map_rejects_bad_arguments():
    import ctypes
    from admmq import _lib
    lib = _lib.load()
    nbk = (ctypes.c_int32 * 2)(3, 2)
    out = (ctypes.c_int32 * 3)()
    assert lib.admmq_debug_chol_step_work(3, 2, nbk, 0, out) == -1     # s past the last block column
    assert lib.admmq_debug_chol_step_work(0, 2, nbk, 6, out) == -1     # launch 0 has 2 x 3 workgroups
    assert lib.admmq_debug_chol_step_work(0, 2, nbk, 5, out) == 6 and out[0] == -1   # (1, 2): the problem has 2 blocks
    with pytest.raises(ValueError):
        _lib.chol_step_work(0, [])


def test_spd_form_switch_range():
    from admmq import _lib
    lib = _lib.load()
    d = lib.admmq_debug_get_spd_form_default()
    assert 0 <= d <= 7
    assert lib.admmq_debug_set_spd_form(-1) != 0 and lib.admmq_debug_set_spd_form(8) != 0
    assert lib.admmq_debug_set_linv_width(4) != 0 and lib.admmq_debug_set_linv_width(12) != 0
    try:
        assert lib.admmq_debug_set_spd_form(2) == 0
        # the launcher's own choice: 2 = 4-column slices with two columns per lane, up to 40 blocks
        assert lib.admmq_debug_linv_width(2) == 2 and lib.admmq_debug_linv_width(40) == 2
        assert lib.admmq_debug_linv_width(41) == 4 and lib.admmq_debug_linv_width(56) == 4
        assert lib.admmq_debug_linv_width(57) == 0 and lib.admmq_debug_linv_width(1) == 0   # no column kernel
        assert lib.admmq_debug_set_linv_width(8) == 0 and lib.admmq_debug_linv_width(9) == 8
        assert lib.admmq_debug_set_linv_width(16) == 0
        assert lib.admmq_debug_linv_width(9) == 16 and lib.admmq_debug_linv_width(50) == 8   # 16 would not fit
        assert lib.admmq_debug_set_spd_form(0) == 0 and lib.admmq_debug_linv_width(9) == 4
    finally:
        assert lib.admmq_debug_set_linv_width(0) == 0 and lib.admmq_debug_set_spd_form(d) == 0
