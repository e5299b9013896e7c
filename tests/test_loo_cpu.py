"""Leave-one-out diagnostics on backend='cpu', and the contract of libgsum_loo.so (no GPU needed)."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.stats

from conftest import ROOT

import gsum_amd as gm  # noqa: E402
from loo_cases import lattice, lattice_alpha, integer_rhs  # noqa: E402


def _brute_case():
    n = 12
    x = np.linspace(0, 1, n)
    K = np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2 / 0.2 ** 2) + 1e-6 * np.eye(n)
    y = np.sin(3 * x) + 0.3
    return n, K, y, 0.3


def test_brute_force_deletion():
    """Delete point i and condition on the others with numpy.linalg.solve, for every i: the closed forms are the same numbers.
    The identity is exact; the gap is the brute force's own conditioning (measured at i in {0, 5, 11}: |d mean| <= 3.5e-10,
    relative d var <= 6e-11), so the bound is 1e-8."""
    n, K, y, m = _brute_case()
    res = gm.loo_from_factor(np.linalg.cholesky(K), y, mean=m, backend="cpu")
    worst_mean = worst_var = 0.0
    for i in range(n):
        o = np.delete(np.arange(n), i)
        s = np.linalg.solve(K[np.ix_(o, o)], np.stack([y[o] - m, K[o, i]], axis=1))
        mean_i = m + K[i, o] @ s[:, 0]
        var_i = K[i, i] - K[i, o] @ s[:, 1]
        worst_mean = max(worst_mean, abs(res.mean[i] - mean_i))
        worst_var = max(worst_var, abs(res.var[i] - var_i) / var_i)
    print(f"brute force: worst |d mean| = {worst_mean:.3g}, worst relative d var = {worst_var:.3g}")
    assert worst_mean <= 1e-8 and worst_var <= 1e-8, (worst_mean, worst_var)
    assert np.array_equal(res.var, 1 / res.precision_diag)
    assert np.allclose(res.error, (y - res.mean) / np.sqrt(res.var), rtol=1e-9, atol=0)
    assert np.allclose(res.logpdf, scipy.stats.norm(res.mean, np.sqrt(res.var)).logpdf(y), rtol=1e-7, atol=1e-7)


@pytest.mark.parametrize("kind", ["subdiag", "ones"])
@pytest.mark.parametrize("n", [1, 2, 129, 257])
def test_exact_lattices(kind, n):
    L, W, p = lattice(kind, n)
    R = integer_rhs(n, 3)
    f = gm.loo.LooFactor(L, backend="cpu")
    np.testing.assert_array_equal(f.precision_diag, p.astype(float))
    np.testing.assert_array_equal(f.solve(R), lattice_alpha(W, R))
    assert f.sum_log_diag == 0.0
    res = f.loo(R[:, 0])
    np.testing.assert_array_equal(res.var, 1.0 / p)
    np.testing.assert_array_equal(res.precision_diag, p.astype(float))


def test_shape_conventions():
    n, K, y, m = _brute_case()
    L = np.linalg.cholesky(K)
    Y = np.stack([y, 2 * y - 1, y ** 2], axis=1)
    one = gm.loo_from_factor(L, y, mean=m, backend="cpu")
    many = gm.loo_from_factor(L, Y, mean=m, backend="cpu")
    assert isinstance(one, gm.LooResult) and one._fields == ("mean", "var", "error", "logpdf", "precision_diag")
    for name in ("mean", "error", "logpdf"):
        assert getattr(one, name).shape == (n,) and getattr(many, name).shape == (n, 3)
        np.testing.assert_allclose(getattr(many, name)[:, 0], getattr(one, name), rtol=1e-9, atol=1e-12)
    assert one.var.shape == many.var.shape == one.precision_diag.shape == (n,)
    np.testing.assert_array_equal(one.var, many.var)
    vec = gm.loo_from_factor(L, y, mean=np.full(n, m), backend="cpu")               # a mean per point
    np.testing.assert_array_equal(vec.mean, one.mean)
    np.testing.assert_array_equal(gm.loo_from_factor(L + np.triu(np.full((n, n), np.nan), 1), y, mean=m, backend="cpu").mean, one.mean)


def test_diagnostic_and_process_on_cpu():
    n, K, y, m = _brute_case()
    ref = gm.loo_from_factor(np.linalg.cholesky(K), y, mean=m, backend="cpu")
    d = gm.Diagnostic(np.full(n, m), K, backend="cpu")
    try:
        got = d.loo(y)
        np.testing.assert_allclose(got.mean, ref.mean, rtol=1e-9, atol=1e-12)
        np.testing.assert_array_equal(d.loo_errors(y), got.error)
        assert d.loo_errors(np.stack([y, y], axis=1)).shape == (n, 2)
    finally:
        d.close()
    with pytest.raises(ValueError):
        d.loo(y)                                                                     # closed
    t = gm.Diagnostic(np.full(n, m), K, df=3, backend="cpu")
    try:
        with pytest.raises(NotImplementedError, match="Student"):
            t.loo(y)
        with pytest.raises(NotImplementedError, match="Student"):
            t.loo_errors(y)
    finally:
        t.close()

    from sklearn.gaussian_process.kernels import RBF
    X = np.linspace(0, 1, n)[:, None]
    Y = np.stack([y, np.cos(2 * X[:, 0])], axis=1)
    gp = gm.ConjugateGaussianProcess(RBF(0.2), nugget=1e-6, optimizer=None, backend="cpu").fit(X, Y)
    cov = float(np.squeeze(gp.cov_factor_)) * (RBF(0.2)(X) + 1e-6 * np.eye(n))
    want = gm.loo_from_factor(np.linalg.cholesky(cov), Y, mean=float(gp.center_[0]), backend="cpu")
    got = gp.loo()
    for name in gm.LooResult._fields:
        np.testing.assert_allclose(getattr(got, name), getattr(want, name), rtol=1e-7, atol=1e-9)
    assert gp.loo(y).mean.shape == (n,)
    with pytest.raises(ValueError):
        gm.ConjugateGaussianProcess(RBF(0.2), backend="cpu").loo()                   # not fitted
    sp = gm.ConjugateStudentProcess(RBF(0.2), nugget=1e-6, optimizer=None, backend="cpu").fit(X, Y)
    with pytest.raises(NotImplementedError):
        sp.loo()


def test_argument_checks():
    n, K, y, m = _brute_case()
    L = np.linalg.cholesky(K)
    for bad_L in (L[:, :-1], L[0], np.zeros((0, 0))):
        with pytest.raises(ValueError):
            gm.loo_from_factor(bad_L, y, backend="cpu")
    for bad_y in (y[:-1], np.zeros((n, 2, 1)), np.zeros((n, 0)), 0.5):
        with pytest.raises(ValueError):
            gm.loo_from_factor(L, bad_y, backend="cpu")
    with pytest.raises(ValueError):
        gm.loo_from_factor(L, y, mean=np.zeros(n - 1), backend="cpu")
    with pytest.raises(ValueError):
        gm.loo_from_factor(L, y, backend="cuda")
    for v in (0.0, -1.0, np.nan, np.inf):
        Lb = L.copy()
        Lb[5, 5] = v
        with pytest.raises(ValueError, match="diagonal entry 5"):
            gm.loo_from_factor(Lb, y, backend="cpu")


def test_public_names():
    for name in ("LooResult", "loo_from_factor"):
        assert name in gm.__all__ and hasattr(gm, name)


def test_loo_library_exports_every_declared_symbol():
    """include/gsum_loo.h is the contract of libgsum_loo.so: every function it declares is exported and bound, nothing else."""
    from gsum_amd import _loo_lib, build
    assert "loo" in build.SIDE
    header = open(os.path.join(ROOT, "include", "gsum_loo.h")).read()
    declared = set(re.findall(r"\b(gsum_loo_[a-z0-9_]+)\s*\(", header))
    assert declared and declared == set(_loo_lib.PROTOTYPES), declared ^ set(_loo_lib.PROTOTYPES)
    path = build.build_loo()
    assert path == _loo_lib.LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("gsum_")}
    assert exported == declared
    lib = _loo_lib.load_library()
    for name in declared:
        assert hasattr(lib, name)


def test_library_refuses_bad_sizes_before_it_touches_a_device():
    """n < 1, k < 1 and null pointers are argument checks on the host: they need no GPU and give a message."""
    import ctypes as C
    from gsum_amd import _loo_lib
    lib = _loo_lib.load_library()
    h = C.c_void_p()
    one = np.ones(1)
    ptr = one.ctypes.data_as(C.POINTER(C.c_double))
    for n in (0, -3):
        assert lib.gsum_loo_open(ptr, n, 0, C.byref(h)) != 0 and h.value is None
        assert f"n must be >= 1, got {n}" in lib.gsum_loo_last_error().decode()
    assert lib.gsum_loo_open(None, 4, 0, C.byref(h)) != 0 and "null pointer" in lib.gsum_loo_last_error().decode()
    assert lib.gsum_loo_solve(None, ptr, 1, ptr) != 0 and "null pointer" in lib.gsum_loo_last_error().decode()
    assert lib.gsum_loo_precision_diag(None, ptr, ptr) != 0 and "null pointer" in lib.gsum_loo_last_error().decode()
    lib.gsum_loo_free(None)
