"""The exact-tie references of tests/exact_pivots.py against LAPACK dpstrf, bit for bit, and the CPU backend against them.

On these inputs every operation of the pivot search is exact, so the whole pivot order, the rank and the factor are determined; almost
every step is an exact multi-way tie that only MAXLOC's first-position rule decides."""
import numpy as np
import pytest
from scipy.linalg.lapack import dpstrf

import gsum_amd as gm
from gsum_amd._cpu import CpuContext
from exact_pivots import dense_pstf2, structured_pstrf, tie_spec

# (n, rank or None for full rank, arrangement): ranks 127 / 128 / 129 / 255 / 256 / 257 stop at the last step of a 128-step panel,
# at its step 0 and at its step 1; 360 and 680 cross panels of LAPACK's own blocking as well
LAPACK_SPECS = [(240, None, "random"), (721, None, "reversed"), (1290, None, "sorted"), (1642, None, "random"),
                (200, 127, "random"), (300, 128, "reversed"), (300, 129, "sorted"), (400, 255, "random"), (500, 256, "reversed"),
                (840, 257, "random"), (500, 360, "random"), (1000, 680, "reversed")]
DENSE_SPECS = [(1, None, "random"), (2, None, "reversed"), (3, None, "sorted"), (129, None, "reversed"), (385, None, "random"),
               (600, 0, "random"), (600, 1, "reversed"), (600, 599, "random"), (900, 800, "sorted")]


def _ids(specs):
    return [f"n{n}_r{'full' if r is None else r}_{a}" for n, r, a in specs]


def _lapack(A):
    c, piv, rank, info = dpstrf(A, tol=-1.0, lower=1)
    return np.tril(c), piv.astype(np.int64) - 1, int(rank), int(info)


def _ties(A, piv, rank):
    """steps j < rank at which the pivot's residual diagonal ties exactly with another remaining row's"""
    L, _, _, _ = dense_pstf2(A)
    d = np.diag(A)[piv].copy()
    acc = np.zeros(len(d))
    ties = 0
    for j in range(rank):
        upd = d[j:] - acc[j:]
        ties += int(np.count_nonzero(upd == upd[0]) > 1)
        acc += L[:, j] ** 2
    return ties


@pytest.mark.parametrize("n,rank,arr", LAPACK_SPECS, ids=_ids(LAPACK_SPECS))
def test_references_equal_lapack_bitwise(n, rank, arr):
    spec = tie_spec(n, rank, arr, seed=n + (rank or 0))
    A = spec.dense()
    assert np.abs(A).max() <= 2.0 ** 20 + 8
    Lc, lp, lr, li = _lapack(A)
    assert lr == spec.rank and li == (0 if lr == n else 1)
    L, p, r, i = dense_pstf2(A)
    ref = structured_pstrf(spec)
    np.testing.assert_array_equal(p, lp)
    np.testing.assert_array_equal(ref.piv, lp)
    assert r == ref.rank == lr and i == ref.info == li
    np.testing.assert_array_equal(L[:, :lr], Lc[:, :lr])
    np.testing.assert_array_equal(ref.dense(n)[:, :lr], Lc[:, :lr])
    assert np.all(Lc[:, :lr] == np.round(Lc[:, :lr]))                 # every entry of the factor is an integer
    # the inputs exercise the tie-break: most steps tie exactly, and taking the lowest row instead of the lowest position differs
    assert _ties(A, lp, lr) >= 0.8 * lr
    if arr == "random" and lr >= 128:
        assert not np.array_equal(structured_pstrf(spec, tiebreak="row").piv, lp)


@pytest.mark.parametrize("n,rank,arr", DENSE_SPECS, ids=_ids(DENSE_SPECS))
def test_structured_equals_dense(n, rank, arr):
    spec = tie_spec(n, rank, arr, seed=3 * n + 1)
    A = spec.dense()
    L, p, r, i = dense_pstf2(A)
    ref = structured_pstrf(spec)
    np.testing.assert_array_equal(ref.piv, p)
    assert (ref.rank, ref.info) == (r, i) == (spec.rank, 0 if spec.rank == n else 1)
    np.testing.assert_array_equal(ref.dense(n)[:, :r], L[:, :r])


def test_negative_diagonal_is_rank_zero():
    spec = tie_spec(300, None, "random", seed=5)
    spec.negate = True
    A = spec.dense()
    _, lp, lr, li = _lapack(A)
    _, p, r, i = dense_pstf2(A)
    ref = structured_pstrf(spec)
    assert lr == r == ref.rank == 0 and li == i == ref.info == 1
    np.testing.assert_array_equal(p, lp)
    np.testing.assert_array_equal(ref.piv, lp)


@pytest.mark.parametrize("n,rank,arr", [(721, None, "reversed"), (840, 257, "random"), (600, 0, "random")])
def test_cpu_backend_matches_references(n, rank, arr):
    spec = tie_spec(n, rank, arr, seed=11 * n)
    A = spec.dense()
    ref = structured_pstrf(spec)
    ctx = CpuContext()
    M = ctx.upload(A)
    info, piv = ctx.pstrf(M)
    np.testing.assert_array_equal(piv, ref.piv)
    if ref.rank < n:
        assert info == ref.rank + 1 and not M.factored
        np.testing.assert_array_equal(M.to_host(), A)
        with pytest.raises(np.linalg.LinAlgError):
            gm.pivoted_cholesky(A, backend="cpu")
        return
    assert info == 0
    Lex = ref.dense(n)
    np.testing.assert_array_equal(M.to_host(), Lex)
    G = gm.pivoted_cholesky(A, backend="cpu")
    np.testing.assert_array_equal(G, Lex[np.argsort(ref.piv)])


@pytest.mark.parametrize("at", [0, 2])
def test_nan_diagonal_contract_cpu(at):
    """dpstrf with a NaN on the diagonal: a stop (info >= 1), A unchanged, LinAlgError from pivoted_cholesky and Diagnostic."""
    A = 2.0 * np.eye(5)
    A[at, at] = np.nan
    ctx = CpuContext()
    M = ctx.upload(A)
    info, _ = ctx.pstrf(M)
    assert info >= 1 and not M.factored
    np.testing.assert_array_equal(M.to_host(), A)
    with pytest.raises(np.linalg.LinAlgError):
        gm.pivoted_cholesky(A, backend="cpu")
    with pytest.raises(np.linalg.LinAlgError):
        gm.Diagnostic(np.zeros(5), A, backend="cpu")
