"""libgsum_refdist.so on the device: column sort, row percentiles and interval coverage against numpy, gsum_amd.GraphicalDiagnostic
on backend='hip' against the reference's drawn numbers (tests/golden/graphical.json), and the size it is for (n = 8192 points,
1000 reference curves) with its timing against the host stage.

Bounds.  Sort: bit-equal (assert_array_equal, which lets -0.0 == +0.0 and NaN == NaN; every nonzero non-NaN value is also compared
by its bits).  Percentiles: 8 eps max(|a|, |b|) with a, b the two order statistics of the row: three roundings of operands no larger
than 2 max(|a|, |b|), doubled.  Coverage: exact.  Golden cases: 1e-9 max|want|, the bound of the reference comparison of the errors
(test_gpu_diagnostics.py), which carries over because order statistics and their convex combinations are 1-Lipschitz in the max
norm of the errors."""
import time

import numpy as np
import pytest
from sklearn.gaussian_process.kernels import RBF

from conftest import record_parity
from graphical_cases import CASES, INTERVALS, BAND_PERC, check_accessors

pytestmark = pytest.mark.gpu

import gsum_amd as gm  # noqa: E402
from gsum_amd import refdist  # noqa: E402

EPS = np.finfo(float).eps
QS = np.array([0.0, 100.0, 2.5, 16.0, 50.0, 84.0, 97.5, 33.3])


def _mix(n, m, seed, nan=False):
    """normal data with ties (a quarter rounded to one decimal), both zeros and both infinities; with ``nan`` NaNs of both signs"""
    rng = np.random.RandomState(seed)
    A = rng.standard_normal((n, m))
    r = rng.uniform(size=A.shape)
    A[r < 0.25] = np.round(A[r < 0.25], 1)
    A[(r >= 0.25) & (r < 0.28)] = 0.0
    A[(r >= 0.28) & (r < 0.31)] = -0.0
    A[(r >= 0.31) & (r < 0.32)] = np.inf
    A[(r >= 0.32) & (r < 0.33)] = -np.inf
    if nan:
        A[(r >= 0.33) & (r < 0.36)] = np.nan
        A[(r >= 0.36) & (r < 0.38)] = -np.nan
    return A


def _assert_sorted_equal(got, want):
    np.testing.assert_array_equal(got, want)
    plain = (want != 0) & ~np.isnan(want)
    np.testing.assert_array_equal(got.view(np.uint64)[plain], want.view(np.uint64)[plain])


SORT_SHAPES = [(n, m) for n in (1, 2, 63, 64, 65, 1000, 8192, 16384, 16385, 40000) for m in (1, 2, 17, 1000) if n <= 16384 or m <= 17]


@pytest.mark.parametrize("n,m", SORT_SHAPES)
def test_sort_columns_bit_equal(n, m):
    A = _mix(n, m, seed=n + m)
    _assert_sorted_equal(refdist.sort_columns(A), np.sort(A, axis=0))


@pytest.mark.parametrize("n,m", [(1, 1), (65, 17), (1000, 2), (16385, 2)])
def test_sort_columns_nan_last(n, m):
    A = _mix(n, m, seed=3 * n + m, nan=True)
    got = refdist.sort_columns(A)
    _assert_sorted_equal(got, np.sort(A, axis=0))
    assert np.array_equal(np.isnan(got), np.isnan(np.sort(A, axis=0)))


def _percentile_bound(A, q):
    """8 eps max(|a|, |b|) per (q, row), a and b the order statistics numpy's 'linear' method combines"""
    S = np.sort(A, axis=1)
    m = A.shape[1]
    v = (m - 1) * (np.asarray(q) / 100)
    i = np.minimum(np.floor(v).astype(int), m - 1)
    i1 = np.minimum(i + 1, m - 1)
    with np.errstate(invalid="ignore"):
        return 8 * EPS * np.maximum(np.abs(S[:, i]), np.abs(S[:, i1])).T


def _assert_percentiles(got, A, q):
    want = np.percentile(A, q, axis=1)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    assert np.all(err <= _percentile_bound(A, q)[ok]), float(err.max())
    return float(err.max()) if err.size else 0.0


@pytest.mark.parametrize("n,m", [(5, 1), (5, 2), (64, 3), (257, 999), (8192, 1000), (40, 16384), (40, 16385)])
def test_row_percentiles(n, m):
    rng = np.random.RandomState(m)
    A = rng.standard_normal((n, m)) * np.exp(rng.uniform(-3, 3, (n, 1)))
    worst = _assert_percentiles(refdist.row_percentiles(A, QS), A, QS)          # every row: nothing sampled
    record_parity(f"refdist_percentiles_n{n}_m{m}", worst_abs=worst)


def test_row_percentiles_ties_and_nan_rows():
    A = _mix(300, 1000, seed=9)
    A = np.where(np.isinf(A), 3.0, A)
    A[7, 11] = np.nan
    A[200, :] = -np.nan
    got = refdist.row_percentiles(A, QS)
    _assert_percentiles(got, A, QS)
    assert np.all(np.isnan(got[:, 7])) and np.all(np.isnan(got[:, 200])) and not np.isnan(got[:, 8]).any()


def _host_coverage(Y, lower, upper):
    return np.stack([np.average((lower < r) & (r < upper), axis=1) for r in Y.T])


@pytest.mark.parametrize("K", [1, 3, 101])
@pytest.mark.parametrize("n,m", [(1, 1), (17, 2), (1000, 17), (2500, 300)])
def test_interval_coverage_exact(n, m, K):
    rng = np.random.RandomState(n + K)
    Y = rng.standard_normal((n, m))
    half = rng.uniform(0, 2.5, (K, 1)) * rng.uniform(0.5, 1.5, (1, n))           # neither nested nor sorted
    lower, upper = -half + 0.1, half + 0.1
    for t in range(min(n * K, 50)):                                              # curves exactly on a bound: strictness
        k, i, j = rng.randint(K), rng.randint(n), rng.randint(m)
        (lower if t % 2 else upper)[k, i] = Y[i, j]
    Y[rng.randint(n), rng.randint(m)] = np.nan
    lower[rng.randint(K), rng.randint(n)] = np.nan
    np.testing.assert_array_equal(refdist.interval_coverage(Y, lower, upper), _host_coverage(Y, lower, upper))


def test_refused_arguments():
    A = np.zeros((3, 4))
    with pytest.raises(ValueError):
        refdist.row_percentiles(A, [101.0])
    with pytest.raises(ValueError):
        refdist.row_percentiles(A, [np.nan])
    with pytest.raises(ValueError):
        refdist.sort_columns(np.zeros((0, 4)))
    with pytest.raises(ValueError):
        refdist.interval_coverage(A, np.zeros((0, 3)), np.zeros((0, 3)))
    M = refdist.device_matrix(A)
    M.free()
    with pytest.raises(ValueError):
        M.sort_columns()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hip_graphical_matches_reference(case):
    g = gm.GraphicalDiagnostic(case["data"], case["mean"], case["cov"], nref=case["nref"], backend="hip")
    try:
        worst = check_accessors(g, case, eigen=False)
        with pytest.raises(NotImplementedError):
            g.qq_data("eigen")
        with pytest.raises(NotImplementedError):
            g.essentials(eigen=True)
    finally:
        g.close()
    record_parity(f"graphical_{case['name']}", worst_rel=worst)


def test_hip_essentials_draws():
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    case = CASES[0]
    g = gm.GraphicalDiagnostic(case["data"], case["mean"], case["cov"], nref=case["nref"], backend="hip")
    try:
        fig, axes = g.essentials(bare=True)
        assert len(axes) == 3 and all(len(ax.lines) > 0 for ax in axes)
        assert len(axes[2].collections) == 2
        plt.close(fig)
        fig, axes = g.essentials(eigen=False)
        assert axes.shape == (2, 3) and not axes[0, 1].axison and not axes[1, 1].axison
        plt.close(fig)
    finally:
        g.close()


def _best_of_three(f):
    f()
    best = np.inf
    for _ in range(3):
        t0 = time.perf_counter()
        out = f()
        best = min(best, time.perf_counter() - t0)
    return best, out


def test_refdist_8192_points_1000_curves():
    """The size this is for.  Numbers: every device result against numpy applied to the SAME device-produced errors.  Time: (a) the
    host stage as it was before this library -- Diagnostic.credible_interval of the 1000 reference curves, np.sort(axis=0) and
    np.percentile(axis=1) of one error kind -- against (b) the device stage from host arrays to host results, best of three after
    a warm-up.  The one assertion on time is (b) < (a)."""
    n, nref = 8192, 1000
    rng = np.random.RandomState(11)
    X = np.sort(rng.uniform(0, 20, n))[:, None]
    cov = RBF(1.0)(X) + 1e-2 * np.eye(n)
    mean = rng.standard_normal(n)
    data = mean[:, None] + np.linalg.cholesky(cov) @ rng.standard_normal((n, 3))
    intervals = np.linspace(0, 1, 101)
    q = np.array([[100 * (1. - b) / 2, 100 * (1. + b) / 2] for b in BAND_PERC]).ravel()      # the class's own percentiles
    g = gm.GraphicalDiagnostic(data, mean, cov, nref=nref, sample_method="cholesky", backend="hip")
    try:
        d = g.diagnostic
        E = d.pivoted_cholesky_errors(g.samples)
        lower, upper = d.udist.interval(np.atleast_2d(intervals).T)

        def device_stage():
            bands = refdist.qq_bands(E, q)
            cov_ = refdist.interval_coverage(g.samples, lower, upper)
            return bands, cov_
        t_dev, (bands, dci) = _best_of_three(device_stage)
        bands2, S = refdist.qq_bands(E, q, return_sorted=True)
        np.testing.assert_array_equal(bands2, bands)                               # a second call: bit-identical
        np.testing.assert_array_equal(refdist.interval_coverage(g.samples, lower, upper), dci)

        t0 = time.perf_counter()
        dci_host = d.credible_interval(g.samples, intervals)
        t_ci = time.perf_counter() - t0
        t0 = time.perf_counter()
        S_host = np.sort(E, axis=0)
        t_sort = time.perf_counter() - t0
        t0 = time.perf_counter()
        bands_host = np.percentile(S_host, q, axis=1)
        t_perc = time.perf_counter() - t0
        t_host = t_ci + t_sort + t_perc

        _assert_sorted_equal(S, S_host)
        worst = _assert_percentiles(bands, S_host, q)
        np.testing.assert_array_equal(dci, dci_host)
        assert bands_host.shape == bands.shape

        # kernel-only times (HIP events) of one upload + QQ bands, one upload + coverage
        M = refdist.device_matrix(E)
        M.qq_bands(q)
        tq = M.times()
        M.free()
        M = refdist.device_matrix(g.samples)
        M.coverage(lower, upper)
        tc = M.times()
        M.free()

        # the accessors of the class at this size go through the same calls
        _, data_sorted, qb = g.qq_data("pivoted_cholesky")
        np.testing.assert_array_equal(qb[:, 0], bands[[0, 2]])
        np.testing.assert_array_equal(qb[:, 1], bands[[1, 3]])
        _assert_sorted_equal(data_sorted, np.sort(d.pivoted_cholesky_errors(data), axis=0))
        dci_data, cb = g.credible_interval_data(intervals, BAND_PERC)
        np.testing.assert_array_equal(dci_data, d.credible_interval(data, intervals))
        np.testing.assert_array_equal(cb[0], np.percentile(dci_host, list(q[:2]), axis=0))
    finally:
        g.close()
    record_parity("refdist_n8192_m1000", host_stage_s=t_host, host_credible_interval_s=t_ci, host_sort_s=t_sort, host_percentile_s=t_perc,
                  device_stage_s=t_dev, percentile_worst_abs=worst, qq_upload_ms=tq["h2d"], qq_transpose_ms=tq["transpose"],
                  qq_column_sort_ms=tq["column_sort"], qq_percentiles_ms=tq["percentiles"], qq_download_ms=tq["d2h"],
                  coverage_upload_ms=tc["h2d"], coverage_kernel_ms=tc["coverage"], coverage_download_ms=tc["d2h"])
    assert t_dev < t_host, (t_dev, t_host)


def test_diagnostic_unchanged_by_a_graphical_diagnostic():
    n = 1024
    rng = np.random.RandomState(5)
    X = np.sort(rng.uniform(0, 10, n))[:, None]
    cov = RBF(0.7)(X) + 1e-4 * np.eye(n)
    Y = rng.standard_normal((n, 7))
    ctx = gm.default_context()
    desc = gm.describe_kernel(RBF(0.7), 1)
    Xs = np.linspace(0, 10, 100)[:, None]

    def run():
        d = gm.Diagnostic(np.zeros(n), cov)
        L, info = ctx.factorize(desc, X, diag_add=1e-4)
        try:
            assert info == 0
            return (d.md_squared(Y), d.pivoted_cholesky_errors(Y), d.cholesky_errors(Y)) + tuple(
                ctx.predict_terms(L, desc, X, Xs, rhs=Y[:, :3], want_cov=True))
        finally:
            L.free()
            d.close()
    before = run()
    g = gm.GraphicalDiagnostic(Y[:, :2], np.zeros(n), cov, nref=50, sample_method="cholesky")
    g.qq_data("cholesky")
    g.credible_interval_data(INTERVALS, BAND_PERC)
    g.close()
    after = run()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
