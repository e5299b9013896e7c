"""The device pivoted Cholesky on exact-tie inputs (tests/exact_pivots.py) against the structured dpstrf reference.

On these inputs every operation of the pivot search is exact, so the device must reproduce dpstrf's whole pivot order, rank and stop
exactly: MAXLOC's first-position tie-break after swaps, the newest move onto a position, stops at every step of a panel, several rows per
lane (n > 32768) and the state a context keeps between calls.  The factor (gs_potrf of P^T A P) is checked against the exact integer
one within the bounds of test_gpu_diagnostics.py; errors and Mahalanobis distances against the exact integer curves."""
import numpy as np
import pytest

from conftest import record_parity
from exact_pivots import structured_pstrf, tie_spec

pytestmark = pytest.mark.gpu

import gsum_amd as gm  # noqa: E402
from gsum_amd import _lib  # noqa: E402

ARRS = ("random", "sorted", "reversed")
FULL_N = [1, 2, 3, 127, 128, 129, 255, 256, 257, 383, 384, 385, 1000, 2049, 4097, 8191]


@pytest.fixture(scope="module")
def ctx():
    return gm.default_context()


@pytest.mark.parametrize("arr", ARRS)
@pytest.mark.parametrize("n", FULL_N)
def test_pstrf_exact_full_rank(ctx, n, arr):
    spec = tie_spec(n, None, arr, seed=n)
    A = spec.dense()
    ref = structured_pstrf(spec)
    M = ctx.upload(A)
    try:
        info, piv = ctx.pstrf(M)
        Lg = M.to_host()
    finally:
        M.free()
    assert info == 0
    np.testing.assert_array_equal(piv, ref.piv)                # every pivot, exactly
    Lex = ref.dense(n)
    amax = np.abs(A).max()
    err = float(np.abs(Lg - Lex).max() / amax)
    rec = float(np.abs(A[np.ix_(piv, piv)] - Lg @ Lg.T).max() / amax)
    nonbitwise = int(np.count_nonzero(Lg != Lex))
    record_parity(f"pstrf_exact_n{n}_{arr}", factor=err, reconstruction=rec, nonbitwise_entries=nonbitwise)
    assert err <= 1e-12, err
    assert rec <= 1e-12, rec


def test_pstrf_exact_several_rows_per_lane(ctx):
    """n = 36000: the first 25 panels have M > 32768, so each of the 128 workgroups owns more than 256 rows.  The factor is checked
    through sqrt_errors (host memory: A and nothing else of n x n)."""
    n, k = 36000, 8
    spec = tie_spec(n, None, "random", seed=36000)
    ref = structured_pstrf(spec)
    A = spec.dense()
    M = ctx.upload(A)
    del A
    try:
        info, piv = ctx.pstrf(M)
        assert info == 0
        np.testing.assert_array_equal(piv, ref.piv)
        rng = np.random.default_rng(1)
        Z = rng.integers(-3, 4, (n, k)).astype(float)
        mean = rng.integers(-5, 6, n).astype(float)
        R = np.empty((n, k))
        R[ref.piv] = ref.sparse(n) @ Z                         # Y - mean = P L Z exactly (integers)
        E, m2 = ctx.sqrt_errors(M, mean[:, None] + R, mean, pivot=True, md2=True)
    finally:
        M.free()
    r1 = float(np.abs(E - Z).max() / np.abs(Z).max())
    s = (Z ** 2).sum(0)
    r2 = float(np.abs(m2 - s).max() / s.max())
    record_parity("pstrf_exact_n36000", errors=r1, md2=r2)
    assert max(r1, r2) <= 1e-10, (r1, r2)


# (name, n, rank, arrangement): ranks 128k - 1, 128k, 128k + 1 stop at the last step of a panel, at its step 0 and at its step 1;
# 2600 of 3000 stops in a late panel with G > 1; n - 1 at the very last step
DEFICIENT = [("zero", 300, 0, "random"), ("negative", 300, None, "random"), ("r1", 300, 1, "reversed"), ("r127", 200, 127, "random"),
             ("r128", 300, 128, "reversed"), ("r129", 300, 129, "sorted"), ("r255", 400, 255, "random"), ("r256", 500, 256, "reversed"),
             ("r257", 700, 257, "random"), ("r2600", 3000, 2600, "random"), ("r999", 1000, 999, "random")]


@pytest.mark.parametrize("name,n,rank,arr", DEFICIENT, ids=[d[0] for d in DEFICIENT])
def test_pstrf_exact_rank_deficient(ctx, name, n, rank, arr):
    spec = tie_spec(n, rank, arr, seed=7 * n + (rank or 0))
    if name == "negative":
        spec.negate = True
    A = spec.dense()
    ref = structured_pstrf(spec)
    assert ref.rank == (0 if name == "negative" else rank)
    M = ctx.upload(A)
    try:
        info, piv = ctx.pstrf(M)
        assert info == ref.rank + 1, (info, ref.rank)
        np.testing.assert_array_equal(piv, ref.piv)
        assert not M.factored
        np.testing.assert_array_equal(M.to_host(), A)           # left bit-identical
    finally:
        M.free()
    with pytest.raises(np.linalg.LinAlgError):
        gm.pivoted_cholesky(A)


def _chunk(n):
    """the column chunk of gs_sqrt_errors_run: kc = floor(2^28 / (8 ldb)), ldb = np + 16 (host/pstrf.hip.h)"""
    np_ = -(-n // 128) * 128
    assert np_ == -(-n // 256) * 256                            # (n chosen so that either padding of gs_padded_order gives np)
    return (256 << 20) // ((np_ + 16) * 8)


@pytest.mark.parametrize("pivot", [True, False])
@pytest.mark.parametrize("kind", ["one", "chunks"])
def test_sqrt_errors_exact(ctx, pivot, kind):
    """Y = mean + P L Z with integer Z: E = Z and md2 = sum z^2 exactly.  pivot = False on the sorted arrangement, whose plain Cholesky
    factor is the integer one.  k = 2 kc + 37: two full chunks and a tail."""
    n = 8191
    kc = _chunk(n)
    assert kc == 4088
    k = 1 if kind == "one" else 2 * kc + 37
    spec = tie_spec(n, None, "random" if pivot else "sorted", seed=81 + pivot)
    A = spec.dense()
    rng = np.random.default_rng(2)
    Z = rng.integers(-3, 4, (n, k)).astype(float)
    mean = rng.integers(-5, 6, n).astype(float)
    M = ctx.upload(A)
    try:
        if pivot:
            ref = structured_pstrf(spec)
            info, piv = ctx.pstrf(M)
            assert info == 0
            np.testing.assert_array_equal(piv, ref.piv)
            R = np.empty((n, k))
            R[ref.piv] = ref.sparse(n) @ Z
        else:
            from scipy.sparse import csr_matrix
            ri, ci, v = spec.factor_coo()
            assert np.all(ri >= ci)
            R = csr_matrix((v, (ri, ci)), shape=(n, n)) @ Z
        Y = mean[:, None] + R
        del R
        E, m2 = ctx.sqrt_errors(M, Y, mean, pivot=pivot, md2=True)
    finally:
        M.free()
    r1 = float(np.abs(E - Z).max() / np.abs(Z).max())
    s = (Z ** 2).sum(0)
    r2 = float(np.abs(m2 - s).max() / s.max())
    record_parity(f"sqrt_errors_exact_{'pstrf' if pivot else 'potrf'}_k{k}", errors=r1, md2=r2)
    assert max(r1, r2) <= 1e-10, (r1, r2)


def test_diagnostic_hip_matches_cpu_on_ties():
    """With the pivots equal, the two backends' pivoted factors and errors agree entry by entry."""
    n = 1000
    spec = tie_spec(n, None, "random", seed=1000)
    A = spec.dense()
    rng = np.random.default_rng(3)
    mean = rng.integers(-5, 6, n).astype(float)
    Y = mean[:, None] + rng.standard_normal((n, 6)) * 100.0
    dh = gm.Diagnostic(mean, A, backend="hip")
    dc = gm.Diagnostic(mean, A, backend="cpu")
    try:
        worst = 0.0
        for name in ("pivoted_cholesky_errors", "md_squared"):
            got, want = np.asarray(getattr(dh, name)(Y)), np.asarray(getattr(dc, name)(Y))
            assert got.shape == want.shape
            r = float(np.abs(got - want).max() / np.abs(want).max())
            assert r <= 1e-10, (name, r)
            worst = max(worst, r)
    finally:
        dh.close()
        dc.close()
    Gh = gm.pivoted_cholesky(A, backend="hip")
    Gc = gm.pivoted_cholesky(A, backend="cpu")
    rg = float(np.abs(Gh - Gc).max() / np.abs(A).max())
    record_parity("diagnostic_hip_vs_cpu_ties", worst_rel=worst, pivoted_cholesky=rg)
    assert rg <= 1e-12, rg


def test_pstrf_state_across_calls():
    """One context: rank-deficient, full rank, a larger order, a smaller order (stat / flags reset, pscratch reused)."""
    c = _lib.HipContext(0)
    try:
        for n, rank, arr in [(1000, 700, "random"), (1000, None, "reversed"), (3000, None, "random"), (500, 300, "random"),
                             (200, None, "sorted"), (600, 129, "random")]:
            spec = tie_spec(n, rank, arr, seed=5 * n + (rank or 1))
            A = spec.dense()
            ref = structured_pstrf(spec)
            M = c.upload(A)
            try:
                info, piv = c.pstrf(M)
            finally:
                M.free()
            assert info == (0 if rank is None else ref.rank + 1), (n, rank, info)
            np.testing.assert_array_equal(piv, ref.piv)
    finally:
        c.close()


@pytest.mark.parametrize("at", [0, 2])
def test_nan_diagonal_contract_hip(ctx, at):
    """A NaN on the diagonal stops the search (info >= 1; LAPACK's rank depends on where the NaN is), leaves A unchanged, and
    pivoted_cholesky / Diagnostic raise LinAlgError."""
    A = 2.0 * np.eye(5)
    A[at, at] = np.nan
    M = ctx.upload(A)
    try:
        info, _ = ctx.pstrf(M)
        assert info >= 1 and not M.factored
        np.testing.assert_array_equal(M.to_host(), A)
    finally:
        M.free()
    with pytest.raises(np.linalg.LinAlgError):
        gm.pivoted_cholesky(A)
    with pytest.raises(np.linalg.LinAlgError):
        gm.Diagnostic(np.zeros(5), A, backend="hip")
