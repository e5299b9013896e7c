"""libgsum_loo.so on the device: exact lattices across every block and merge edge, random SPD factors against long-double truth
with scipy's route as the yardstick, agreement of Diagnostic.loo / ConjugateGaussianProcess.loo with backend='cpu', curve
chunking, determinism and refusals."""
import numpy as np
import pytest

from conftest import record_parity

import gsum_amd as gm  # noqa: E402
from gsum_amd.loo import LooFactor  # noqa: E402
import loo_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["subdiag", "ones"])
@pytest.mark.parametrize("n", lc.LATTICE_SIZES)
def test_lattices_bit_equal(kind, n):
    L, W, p = lc.lattice(kind, n)
    R = lc.integer_rhs(n, 5)
    f = LooFactor(L, backend="hip")
    try:
        np.testing.assert_array_equal(f.precision_diag, p.astype(float))
        assert f.sum_log_diag == 0.0
        np.testing.assert_array_equal(f.solve(R), lc.lattice_alpha(W, R))
        res = f.loo(R[:, 0], mean=1.0)
        np.testing.assert_array_equal(res.var, 1.0 / p)
    finally:
        f.free()


@pytest.mark.parametrize("name", list(lc.CLASSES))
@pytest.mark.parametrize("n", lc.RANDOM_SIZES)
def test_random_factors_against_long_double(name, n):
    """The device's p and alpha from numpy's float64 factor L, against the long-double inverse of that same L; scipy's
    solve_triangular route (backend='cpu') on the same L is the yardstick: within 4x its error, floor 64 * 2^-53 (a different but
    equally valid summation order over at most 641 terms)."""
    L, R, p_true, a_true = lc.factor_case(name, n)
    cond = float(np.linalg.cond(lc.spd(name, n)))
    if name in lc.CONDITIONED:
        assert cond <= lc.COND_LIMIT, cond
    c = LooFactor(L, backend="cpu")
    d = LooFactor(L, backend="hip")
    try:
        sp, sa = lc.rel_p(c.precision_diag, p_true), lc.rel_a(c.solve(R), a_true)
        dp, da = lc.rel_p(d.precision_diag, p_true), lc.rel_a(d.solve(R), a_true)
        sld = abs(d.sum_log_diag - np.sum(np.log(np.diag(L))))
    finally:
        d.free()
    record_parity(f"loo_factor_{name}_n{n}", cond=cond, device_p=dp, scipy_p=sp, device_alpha=da, scipy_alpha=sa, sum_log_diag_abs=float(sld))
    assert dp <= max(4 * sp, lc.FLOOR), (dp, sp)
    assert da <= max(4 * sa, lc.FLOOR), (da, sa)
    assert sld <= 1e-12 * max(1.0, np.sum(np.abs(np.log(np.diag(L))))), sld


def _k_truth(K, R):
    """(p, alpha) of K^-1 in long double, from the long-double Cholesky factor of K."""
    return lc.truth_from_factor_ld(lc.cholesky_ld(K), R)


@pytest.mark.parametrize("name", list(lc.CONDITIONED))
def test_diagnostic_agrees_with_cpu_backend(name):
    """Diagnostic.loo on 'hip' against backend='cpu' on the same covariance.  The two factors differ by the device Cholesky, so the
    bound is 4x the distance of numpy's own float64 route from the long-double truth of K (computed here), floor 64 * 2^-53; the
    distance and the gap are relative in p.  The same figures for alpha = K^-1 r are recorded, not asserted: at matern52 the gap
    in alpha was measured at 9.3e-13 = 4.6x numpy's distance (2.0e-13), all of it the device Cholesky factor's own distance from
    the truth (9.0e-13); on one and the same factor the leave-one-out kernels stay within 2x scipy's route
    (test_random_factors_against_long_double)."""
    n = 257
    K = np.array(lc.spd(name, n))
    Y = lc.curves(n, 3, seed=2) + 0.3
    mean = np.full(n, 0.3)
    p_true, a_true = _k_truth(K, Y - 0.3)
    c = gm.Diagnostic(mean, K, backend="cpu")
    d = gm.Diagnostic(mean, K, backend="hip")
    try:
        rc, rd = c.loo(Y), d.loo(Y)
        np.testing.assert_array_equal(d.loo_errors(Y), rd.error)
        np.testing.assert_array_equal(d.loo(Y[:, 1]).mean, rd.mean[:, 1])
    finally:
        c.close()
        d.close()
    assert d._loo is None
    yard_p = lc.rel_p(rc.precision_diag, p_true)
    ac = rc.error * np.sqrt(rc.precision_diag)[:, None]             # a = error sqrt(p): two roundings, no cancellation
    yard_a = lc.rel_a(ac, a_true)
    ad = rd.error * np.sqrt(rd.precision_diag)[:, None]
    gap_p = float(np.max(np.abs(rd.precision_diag - rc.precision_diag) / rc.precision_diag))
    gap_a = float(np.max(np.abs(ad - ac)) / np.max(np.abs(ac)))
    dev_p, dev_a = lc.rel_p(rd.precision_diag, p_true), lc.rel_a(ad, a_true)
    record_parity(f"loo_diagnostic_{name}_n{n}", gap_p=gap_p, numpy_p=yard_p, device_p=dev_p, gap_alpha=gap_a, numpy_alpha=yard_a, device_alpha=dev_a)
    assert gap_p <= max(4 * yard_p, lc.FLOOR), (gap_p, yard_p)
    for got, want in zip(rd, rc):
        assert got.shape == want.shape


def test_process_agrees_with_cpu_backend():
    """ConjugateGaussianProcess.loo on 'hip' against backend='cpu' (fixed kernel, so both fit the same process): the same bound,
    from the long-double truth of the cpu process's covariance."""
    from sklearn.gaussian_process.kernels import Matern
    n = 129
    X = np.arange(n, dtype=float)[:, None]
    Y = lc.curves(n, 3, seed=3)
    kern = Matern(length_scale=4.0, nu=2.5)
    gc = gm.ConjugateGaussianProcess(kern, nugget=1e-8, optimizer=None, backend="cpu").fit(X, Y)
    gd = gm.ConjugateGaussianProcess(kern, nugget=1e-8, optimizer=None, backend="hip").fit(X, Y)
    rc, rd = gc.loo(), gd.loo()
    K = float(np.squeeze(gc.cov_factor_)) * (kern(X) + 1e-8 * np.eye(n))
    p_true, _ = _k_truth(K, Y)
    yard = lc.rel_p(rc.precision_diag, p_true)
    gap = float(np.max(np.abs(rd.precision_diag - rc.precision_diag) / rc.precision_diag))
    gap_mean = float(np.max(np.abs(rd.mean - rc.mean)) / np.max(np.abs(rc.mean)))
    record_parity(f"loo_process_matern52_n{n}", gap_p=gap, numpy_p=yard, gap_mean=gap_mean)
    assert gap <= max(4 * yard, lc.FLOOR), (gap, yard)
    assert gap_mean <= max(4 * yard, lc.FLOOR), (gap_mean, yard)
    assert rd.mean.shape == (n, 3) and gd.loo(Y[:, 0]).mean.shape == (n,)
    with pytest.raises(NotImplementedError):
        gm.ConjugateStudentProcess(kern, nugget=1e-8, optimizer=None, backend="hip").fit(X, Y).loo()


@pytest.mark.parametrize("n", [129, 385])
def test_curves_in_one_call_equal_one_at_a_time(n):
    """k in {1, 16, 17, 33} curves in one call are the same curves one at a time, bit for bit; two identical calls are bit-equal,
    and so are two handles on the same factor."""
    L = lc.factor_case("matern52", 641)[0][:n, :n]                  # a leading block of a factor is a factor
    R = lc.curves(n, 33, seed=4)
    f, g = LooFactor(L, backend="hip"), LooFactor(L, backend="hip")
    try:
        singles = np.concatenate([f.solve(R[:, j:j + 1]) for j in range(33)], axis=1)
        for k in (1, 16, 17, 33):
            np.testing.assert_array_equal(f.solve(R[:, :k]), singles[:, :k])
        np.testing.assert_array_equal(f.solve(R), f.solve(R))
        np.testing.assert_array_equal(g.precision_diag, f.precision_diag)
        np.testing.assert_array_equal(g.solve(R), singles)
        assert g.sum_log_diag == f.sum_log_diag
    finally:
        f.free()
        g.free()


def test_more_curves_than_one_chunk():
    """600 curves cross the library's internal column chunk (512): every column equals its single-curve solve."""
    n = 129
    L = lc.factor_case("rbf", n)[0]
    R = lc.curves(n, 600, seed=5)
    f = LooFactor(L, backend="hip")
    try:
        A = f.solve(R)
        for j in (0, 511, 512, 599):
            np.testing.assert_array_equal(A[:, j:j + 1], f.solve(R[:, j:j + 1]))
        t = f.times()
        assert set(t) == {"upload", "inverse", "reduce", "h2d", "solve", "d2h"} and t["inverse"] > 0 and t["solve"] > 0
    finally:
        f.free()


@pytest.mark.parametrize("bad", [0.0, -2.0, float("nan"), float("inf")])
@pytest.mark.parametrize("row", [0, 130, 256])
def test_bad_diagonal_is_refused_with_a_message(bad, row):
    """The diagonal is checked inside the first kernel and reported through last_error; the next valid handle works."""
    n = 257
    L, W, p = lc.lattice("ones", n)
    Lb = L.copy()
    Lb[row, row] = bad
    with pytest.raises(ValueError, match=f"diagonal entry {row} is not a finite positive number"):
        LooFactor(Lb, backend="hip")
    f = LooFactor(L, backend="hip")
    try:
        np.testing.assert_array_equal(f.precision_diag, p.astype(float))
    finally:
        f.free()


def test_argument_refusals_on_the_device():
    import ctypes as C
    from gsum_amd import _loo_lib
    L, W, p = lc.lattice("ones", 5)
    f = _loo_lib.DeviceLoo(0, L)
    try:
        lib = f._lib
        R = np.ones((5, 1))
        ptr = R.ctypes.data_as(C.POINTER(C.c_double))
        for k in (0, -1):
            assert lib.gsum_loo_solve(f._h, ptr, k, ptr) != 0
            assert f"k must be >= 1, got {k}" in lib.gsum_loo_last_error().decode()
        with pytest.raises(ValueError):
            f.solve(np.ones((4, 1)))
        # an order whose padded matrices cannot fit any device is refused by the memory check, before L is read
        h = C.c_void_p()
        assert lib.gsum_loo_open(ptr, 1 << 19, 0, C.byref(h)) != 0 and h.value is None
        assert "MiB of device memory" in lib.gsum_loo_last_error().decode()
        np.testing.assert_array_equal(f.solve(R), lc.lattice_alpha(W, R))
    finally:
        f.free()
    with pytest.raises(ValueError):
        f.solve(np.ones((5, 1)))                                    # freed
