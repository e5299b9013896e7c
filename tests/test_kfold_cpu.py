"""Leave-group-out predictions on backend='cpu' (loo.py): exact lattices and plumbing, the closed forms that need no truth,
independence, accuracy against the long-double brute force of kfold_cases.py, the model level, the fold arguments and the host-side
refusals of libgsum_loo.so (no device needed)."""
import ctypes as C

import numpy as np
import pytest

import gsum_amd as gm  # noqa: E402
from gsum_amd.loo import LooFactor, normalise_folds  # noqa: E402
import kfold_cases as kc  # noqa: E402
import loo_cases as lc  # noqa: E402


@pytest.mark.parametrize("kind", ["subdiag", "ones"])
@pytest.mark.parametrize("n", lc.LATTICE_SIZES)
def test_precision_block_of_lattices_bit_equal(kind, n):
    kc.check_precision_block_lattice(kind, n, "cpu")


@pytest.mark.parametrize("lay", kc.LAYOUTS)
@pytest.mark.parametrize("n", [129, 641])
def test_exact_plumbing(n, lay):
    kc.check_plumbing(n, lay, "cpu")


@pytest.mark.parametrize("name", list(lc.CLASSES))
@pytest.mark.parametrize("n", kc.TRUTH_SIZES)
def test_closed_forms_without_a_truth(name, n):
    bound = kc.FLOOR * float(np.linalg.cond(lc.spd(name, n)))
    for what, d in kc.closed_form_gaps(name, n, "cpu").items():
        assert d <= bound, (what, d, bound)


@pytest.mark.parametrize("n", [129, 385])
def test_independence_bitwise(n):
    kc.check_independence(n, "cpu")


@pytest.mark.parametrize("lay", kc.TRUTH_LAYOUTS)
@pytest.mark.parametrize("name", list(lc.CLASSES))
@pytest.mark.parametrize("n", kc.TRUTH_SIZES)
def test_accuracy_against_long_double(name, n, lay):
    """The cpu backend against the brute force, within FLOOR * cond(K) in the norms of kfold_cases.distances."""
    L, R, groups, truth = kc.truth_case(name, n, lay)
    bound = kc.FLOOR * float(np.linalg.cond(lc.spd(name, n)))
    f = LooFactor(L, backend="cpu")
    try:
        d = kc.distances(kc.raw_folds(f, groups, R), truth)
    finally:
        f.free()
    print(name, n, lay, d, bound)
    for what, v in d.items():
        assert v <= bound, (what, v, bound)


def test_brute_force_is_the_leave_one_out_on_singletons():
    """The long-double truth itself, on singletons, against loo_cases' long-double leave-one-out from the same factor."""
    L, R, p, a = lc.factor_case("matern52", 129)
    resid, var, md2, logdet = kc.brute_force_ld(L, R, kc.layout("singletons", 129))
    assert np.max(np.abs(var * p - 1)) < 1e-13
    assert np.max(np.abs(resid - a / p[:, None])) / np.max(np.abs(a / p[:, None])) < 1e-13
    assert np.max(np.abs(md2 - resid ** 2 / var[:, None])) < 1e-13 * np.max(md2)
    assert np.max(np.abs(logdet - np.log(var))) < 1e-13


def test_model_level():
    n = 129
    K = np.array(lc.spd("matern52", n))
    Y = lc.curves(n, 3, seed=2) + 0.3
    mean = np.full(n, 0.3)
    folds = gm.make_folds(n, 4, "interleaved")
    d = gm.Diagnostic(mean, K, backend="cpu")
    try:
        got = d.kfold(Y, folds)
        assert d._loo is not None
        want = gm.kfold_from_factor(d._L.to_host(), Y, folds, mean=mean, backend="cpu")
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        held = d._loo
        d.loo(Y)
        assert d._loo is held                                       # one resident inverse for both
        assert d.kfold(Y[:, 0], 5).mean.shape == (n,)
    finally:
        d.close()
    with pytest.raises(ValueError):
        d.kfold(Y, folds)                                           # closed
    t = gm.Diagnostic(mean, K, df=3, backend="cpu")
    try:
        with pytest.raises(NotImplementedError, match="Student"):
            t.kfold(Y, folds)
    finally:
        t.close()

    from sklearn.gaussian_process.kernels import Matern
    X = np.arange(n, dtype=float)[:, None]
    kern = Matern(length_scale=4.0, nu=2.5)
    gp = gm.ConjugateGaussianProcess(kern, nugget=1e-8, optimizer=None, backend="cpu").fit(X, Y)
    L = np.sqrt(float(np.squeeze(gp.cov_factor_))) * gp._L_dev.to_host()
    want = gm.kfold_from_factor(L, Y, folds, mean=gp.mean(X), backend="cpu")
    for g, w in zip(gp.kfold(folds), want):
        np.testing.assert_array_equal(g, w)
    assert gp.kfold(3, y=Y[:, 0]).mean.shape == (n,)
    with pytest.raises(ValueError):
        gm.ConjugateGaussianProcess(kern, backend="cpu").kfold(3)   # not fitted
    with pytest.raises(NotImplementedError):
        gm.ConjugateStudentProcess(kern, nugget=1e-8, optimizer=None, backend="cpu").fit(X, Y).kfold(3)


def test_fold_arguments():
    n = 10
    ptr, idx, of = normalise_folds(3, n)
    np.testing.assert_array_equal(ptr, [0, 4, 7, 10])
    np.testing.assert_array_equal(idx, np.arange(n))
    np.testing.assert_array_equal(of, [0, 0, 0, 0, 1, 1, 1, 2, 2, 2])
    lab = np.array([7, 7, -1, 3, 3, 3, -1, 7, 9, 9])
    ptr, idx, of = normalise_folds(lab, n)
    np.testing.assert_array_equal(of, [2, 2, 0, 1, 1, 1, 0, 2, 3, 3])                        # numbered by ascending label
    np.testing.assert_array_equal(ptr, [0, 2, 5, 8, 10])
    np.testing.assert_array_equal(idx, [2, 6, 3, 4, 5, 0, 1, 7, 8, 9])
    ptr, idx, of = normalise_folds([[9, 0], [1, 2, 3, 4], np.array([8, 7, 6, 5])], n)
    np.testing.assert_array_equal(ptr, [0, 2, 6, 10])
    np.testing.assert_array_equal(of, [0, 1, 1, 1, 1, 2, 2, 2, 2, 0])
    ptr, idx, of = normalise_folds([[i] for i in range(n)], n)                               # n singletons: a rectangular list
    np.testing.assert_array_equal(of, np.arange(n))
    for bad in (0, n + 1, -2, True, 2.5, "ab", None, np.zeros(n), np.zeros(n - 1, dtype=int), [[0, 1], [2, 3]], [[0, 1, 2, 3, 4], [4, 5, 6, 7, 8, 9]],
                [[0, 1, 2, 3, 4], [], [5, 6, 7, 8, 9]], [[0, 1, 2, 3, 4], [5, 6, 7, 8, 10]], [[0, 1, 2, 3, 4], [5, 6, 7, 8, -1]],
                [[0.0, 1.0], [2.0]], []):
        with pytest.raises(ValueError):
            normalise_folds(bad, n)

    for k in (1, 3, 10):
        for kind in ("blocks", "interleaved", "random"):
            lab = gm.make_folds(n, k, kind, random_state=4)
            assert lab.shape == (n,) and sorted(np.bincount(lab).tolist(), reverse=True) == [len(a) for a in np.array_split(np.arange(n), k)]
    np.testing.assert_array_equal(gm.make_folds(7, 3, "interleaved"), [0, 1, 2, 0, 1, 2, 0])
    np.testing.assert_array_equal(gm.make_folds(7, 3, "random", random_state=1), gm.make_folds(7, 3, "random", random_state=1))
    for args in ((n, 0), (n, n + 1), (0, 1), (n, 2, "spiral")):
        with pytest.raises(ValueError):
            gm.make_folds(*args)


def test_argument_refusals():
    n = 129
    L, R, _, _ = lc.factor_case("rbf", n)
    for bad_y in (R[:-1], np.zeros((n, 2, 1)), np.zeros((n, 0)), 0.5):
        with pytest.raises(ValueError):
            gm.kfold_from_factor(L, bad_y, 3, backend="cpu")
    with pytest.raises(ValueError):
        gm.kfold_from_factor(L, R, 3, mean=np.zeros(n - 1), backend="cpu")
    with pytest.raises(ValueError):
        gm.kfold_from_factor(L, R, n + 1, backend="cpu")
    f = LooFactor(L, backend="cpu")
    try:
        for bad in ([], [0, 0], [n], [-1], [[0, 1]], [0.5]):
            with pytest.raises(ValueError):
                f.precision_block(bad)
    finally:
        f.free()


def test_a_block_that_does_not_factor_names_its_group():
    """A diagonal factor with one entry of 1e-200: that point's precision overflows to inf, so its group's block does not factor."""
    n = 12
    d = np.ones(n)
    d[7] = 1e-200
    with np.errstate(all="ignore"):
        f = LooFactor(np.diag(d), backend="cpu")
    try:
        with np.errstate(all="ignore"), pytest.raises(np.linalg.LinAlgError, match="group 2 "):
            f.folds(np.ones(n), 4)
    finally:
        f.free()


def test_public_names():
    for name in ("FoldResult", "kfold_from_factor", "make_folds"):
        assert name in gm.__all__ and hasattr(gm, name)
    assert gm.FoldResult._fields == ("mean", "var", "error", "md2", "logpdf", "fold_of")
    assert gm.LooResult._fields == ("mean", "var", "error", "logpdf", "precision_diag")
    for name in ("folds", "precision_block"):
        assert hasattr(LooFactor, name)


def test_library_refuses_fold_arguments_before_it_touches_a_device():
    """Bad sizes and null pointers of the new entry points are argument checks on the host: they need no GPU and give a message."""
    from gsum_amd import _loo_lib
    lib = _loo_lib.load_library()
    one = np.ones(1)
    ptr = one.ctypes.data_as(C.POINTER(C.c_double))
    ip = np.zeros(2, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))

    def err():
        return lib.gsum_loo_last_error().decode()

    for nf in (0, -2):
        assert lib.gsum_loo_folds(None, ip, ip, nf, ptr, 1, ptr, ptr, ptr, ptr) != 0 and f"n_folds must be >= 1, got {nf}" in err()
    for k in (0, -1):
        assert lib.gsum_loo_folds(None, ip, ip, 1, ptr, k, ptr, ptr, ptr, ptr) != 0 and f"k must be >= 1, got {k}" in err()
    assert lib.gsum_loo_folds(None, ip, ip, 1, ptr, 1, ptr, ptr, ptr, ptr) != 0 and "null pointer" in err()
    for g in (0, -5):
        assert lib.gsum_loo_precision_block(None, ip, g, ptr) != 0 and f"g must be >= 1, got {g}" in err()
    assert lib.gsum_loo_precision_block(None, ip, 1, ptr) != 0 and "null pointer" in err()
    assert lib.gsum_loo_fold_times(None, ptr, 0) != 0 and "null pointer" in err()
    assert lib.gsum_loo_fold_budget(None, 0) != 0 and "null pointer" in err()
