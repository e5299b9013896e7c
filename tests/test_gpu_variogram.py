"""VariogramFourthRoot on the device (libgsum_vario.so): the reference's fixture, hip against cpu, exact bins, reproducibility, the
correlation map against mpmath, a large case, and the product context left untouched.  Run with -m gpu on an MI355X."""
import time
import warnings

import numpy as np
import pytest
from sklearn.gaussian_process.kernels import RBF

import gsum_amd as gm
from conftest import load_golden
from test_variogram_cpu import A, check_case, cov_close, same_nan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("variogram.json")["cases"]


def rule_bounds(X):
    N = len(X)
    return np.linspace(0, np.max(np.linalg.norm(X, axis=-1)), int(np.ceil((N * (N - 1) / 2.) ** (1. / 3))))


def test_hip_matches_the_reference(golden):
    for case in golden:
        check_case(case, "hip")


@pytest.mark.parametrize("N,d,nc,seed", [(300, 1, 1, 0), (300, 2, 3, 1), (500, 3, 8, 2), (500, 1, 2, 3)])
def test_hip_against_cpu(N, d, nc, seed):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, d))
    z = rng.standard_normal((nc, N)).cumsum(axis=1) / np.sqrt(N)
    bounds = np.concatenate([[0.001, 0.003], np.linspace(0.01, 0.9 * np.sqrt(d), 40)])   # bins from 1 to ~10^4 pairs
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        h = gm.VariogramFourthRoot(X, z, bounds, backend="hip")
        c = gm.VariogramFourthRoot(X, z, bounds, backend="cpu")
        np.testing.assert_array_equal(h.bin_counts, c.bin_counts)
        assert h.bin_counts.max() > 1000 and h.bin_counts[h.bin_counts > 0].min() < 500
        np.testing.assert_allclose(h.bin_locations, c.bin_locations, rtol=1e-12)
        np.testing.assert_allclose(h.gamma_tilde, c.gamma_tilde, rtol=1e-11)
        # diagonal bins up to ~2000 pairs on the host; off-diagonal pairs including the largest bin against a small one
        small = [b for b in np.flatnonzero(h.bin_counts) if h.bin_counts[b] <= 2000 // nc + 50]
        pick = small[:: max(1, len(small) // 5)]
        big, tiny = int(np.argmax(h.bin_counts)), int(small[0])
        pairs = [(b, b) for b in pick] + [(big, tiny), (tiny, big), (pick[-1], pick[0])]
        got = np.array([np.broadcast_to(h.cov(a, b), (nc,)) for a, b in pairs])
        want = np.array([np.broadcast_to(c.cov(a, b), (nc,)) for a, b in pairs])
        cov_close(got, want)
        h.close()


def test_bins_match_numpy_on_the_bounds():
    """bounds = every distinct distance numpy computes: a distance one ulp off would change its bin"""
    rng = np.random.RandomState(7)
    for N, d in ((150, 1), (120, 3), (100, 9), (90, 17)):
        X = np.round(rng.uniform(0, 4, (N, d)), 1)
        ti, tj = np.tril_indices(N, -1)
        h = np.linalg.norm(X[:, None, :] - X, axis=-1)[ti, tj]
        bounds = np.unique(h)[:32000]
        v = gm.VariogramFourthRoot(X, rng.standard_normal(N), bounds, backend="hip")
        np.testing.assert_array_equal(v.bin_counts, np.bincount(np.digitize(h, bounds), minlength=len(bounds) + 1))
        v.close()
    g = np.arange(9.0)
    X = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    ti, tj = np.tril_indices(len(X), -1)
    h = np.linalg.norm(X[:, None, :] - X, axis=-1)[ti, tj]
    bounds = np.arange(0.0, 13.0)
    v = gm.VariogramFourthRoot(X, np.sin(X[:, 0]), bounds, backend="hip")
    np.testing.assert_array_equal(v.bin_counts, np.bincount(np.digitize(h, bounds), minlength=len(bounds) + 1))


def test_compute_is_bitwise_reproducible():
    rng = np.random.RandomState(3)
    X = np.sort(rng.uniform(0, 1, 700))[:, None]
    z = rng.standard_normal((5, 700)).cumsum(axis=1)
    v = gm.VariogramFourthRoot(X, z, rule_bounds(X), backend="hip")
    a, b = v.compute(), v.compute()
    w = gm.VariogramFourthRoot(X, z, rule_bounds(X), backend="hip")
    c = w.compute()
    np.testing.assert_array_equal(v.gamma_tilde, w.gamma_tilde)
    for x, y, u in zip(a, b, c):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, u)


def test_device_corr_against_mpmath():
    mp = pytest.importorskip("mpmath")
    from gsum_amd._vario_lib import device_corr
    cf = gm.VariogramFourthRoot.corr_factor
    rng = np.random.RandomState(11)
    k = np.arange(1, 53)
    rho = np.concatenate([rng.uniform(-1, 1, 9000), 1 - 2.0 ** -k, -(1 - 2.0 ** -k), np.linspace(-1, 1, 801),
                          [0.0, -0.0, 1.0, -1.0, 1.5, -3.0, np.inf, -np.inf, np.nan, np.sqrt(0.5), np.nextafter(np.sqrt(0.5), 0)]])
    got = device_corr(rho, cf)
    mp.mp.dps = 30
    g = mp.gamma(mp.mpf(3) / 4) ** 2
    cf_mp = g / (mp.sqrt(mp.pi) - g)
    worst = 0.0
    for r, c in zip(rho, got):
        if np.isnan(r):
            assert np.isnan(c)
        elif r >= 1:
            assert c == 1.0
        elif r <= -1:
            assert c == -1.0
        else:
            want = cf_mp * (mp.hyp2f1(-0.25, -0.25, 0.5, mp.mpf(float(r)) ** 2) - 1)
            worst = max(worst, abs(float(mp.mpf(float(c)) - want)))
    print(f"worst |corr - mpmath| = {worst:.2e}")
    assert worst <= 4e-15


def test_large_case_finishes():
    N = 2000
    rng = np.random.RandomState(4)
    X = np.sort(rng.uniform(0, 1, N))[:, None]
    z = rng.standard_normal((4, N)).cumsum(axis=1) / np.sqrt(N)
    bounds = rule_bounds(X)
    t0 = time.perf_counter()
    v, loc, gam, lo, up = gm.Diagnostic.variogram(X, z, bounds, backend="hip")
    dt = time.perf_counter() - t0
    print(f"N = 2000, 4 curves, {v.Nb} bins: {dt:.3f} s")
    assert gam.shape == lo.shape == up.shape == (len(bounds) + 1, 4) and loc.shape == (len(bounds) + 1,)
    full = v.bin_counts > 0
    np.testing.assert_array_equal(np.isfinite(gam).all(axis=1), full)
    assert dt < 10.0


def test_closed_object_and_library_refusals():
    from gsum_amd._vario_lib import DeviceVariogram
    X = np.linspace(0, 1, 20)[:, None]
    with pytest.raises(ValueError, match="non-decreasing"):
        DeviceVariogram(0, X, np.sin(X.T), np.array([0.5, 0.2]))
    with pytest.raises(ValueError, match="65535"):
        DeviceVariogram(0, np.zeros((65536, 1)), np.zeros((1, 65536)), np.array([0.5]))
    v = gm.VariogramFourthRoot(X, np.sin(X[:, 0]), np.linspace(0, 1, 5), backend="hip")
    v.close()
    with pytest.raises(ValueError, match="closed"):
        v.compute()


def test_nan_in_z_propagates():
    X = np.linspace(0, 1, 40)[:, None]
    z = np.vstack([np.sin(5 * X[:, 0]), np.cos(5 * X[:, 0])])
    z[1, 7] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        h = gm.VariogramFourthRoot(X, z, np.linspace(0, 1, 8), backend="hip").compute()
        c = gm.VariogramFourthRoot(X, z, np.linspace(0, 1, 8), backend="cpu").compute()
    for a, b in zip(h, c):
        same_nan(a, b)


def test_product_context_unchanged_by_a_variogram():
    ctx = gm.default_context()
    n, m = 1024, 200
    rng = np.random.RandomState(5)
    X = np.sort(rng.uniform(0, 10, n))[:, None]
    Xs = np.linspace(0, 10, m)[:, None]
    rhs = rng.standard_normal((n, 3))
    desc = gm.describe_kernel(RBF(0.7), 1)

    def run():
        L, info = ctx.factorize(desc, X, diag_add=1e-6)
        try:
            assert info == 0
            return ctx.predict_terms(L, desc, X, Xs, rhs=rhs, want_cov=True)
        finally:
            L.free()
    before = run()
    v = gm.VariogramFourthRoot(X, rhs.T, rule_bounds(X), backend="hip")
    v.compute()
    v.close()
    after = run()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
