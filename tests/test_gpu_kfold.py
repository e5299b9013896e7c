"""Leave-group-out predictions of libgsum_loo.so on the device: exact lattices and plumbing across the block, tile and fragment
edges, the closed forms that need no truth, independence of a group from its call (other groups, order, curves, chunks), accuracy
against the long-double brute force with backend='cpu' as the yardstick, the model level and refusals."""
import ctypes as C

import numpy as np
import pytest

from conftest import record_parity

import gsum_amd as gm  # noqa: E402
from gsum_amd.loo import LooFactor, normalise_folds  # noqa: E402
import kfold_cases as kc  # noqa: E402
import loo_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["subdiag", "ones"])
@pytest.mark.parametrize("n", lc.LATTICE_SIZES)
def test_precision_block_of_lattices_bit_equal(kind, n):
    kc.check_precision_block_lattice(kind, n, "hip")


@pytest.mark.parametrize("lay", kc.LAYOUTS)
@pytest.mark.parametrize("n", [129, 641])
def test_exact_plumbing(n, lay):
    kc.check_plumbing(n, lay, "hip")


@pytest.mark.parametrize("name", list(lc.CLASSES))
@pytest.mark.parametrize("n", kc.TRUTH_SIZES)
def test_closed_forms_without_a_truth(name, n):
    """Singletons against the object's own leave-one-out and the one-group layout against r, diag(K), 2 sum_log_diag and r^T a:
    the device's distance is at most 4x the cpu backend's distance between the same two of its own results, floor 64 * 2^-53.

    Measured 2026-10-19 on an MI355X: every figure inside the bound; one_logdet of rbf2d at n = 257 is 2.8e-16 (cpu 5.3e-15)."""
    cpu = kc.closed_form_gaps(name, n, "cpu")
    dev = kc.closed_form_gaps(name, n, "hip")
    record_parity(f"kfold_closed_{name}_n{n}", **{f"device_{k}": v for k, v in dev.items()}, **{f"cpu_{k}": v for k, v in cpu.items()})
    for what in dev:
        assert dev[what] <= max(4 * cpu[what], kc.FLOOR), (what, dev[what], cpu[what])


@pytest.mark.parametrize("n", [129, 385])
def test_independence_bitwise(n):
    kc.check_independence(n, "hip")


@pytest.mark.parametrize("lay", ["random_sizes", "blocks5", "singletons"])
def test_chunks_do_not_change_a_bit(lay):
    """A budget that cuts the groups into several chunks (with another common leading dimension) against the single chunk."""
    n = 641
    L, R, _, _ = lc.factor_case("matern52", n)
    groups = kc.layout(lay, n)
    f = LooFactor(L, backend="hip")
    try:
        whole = kc.raw_folds(f, groups, R)
        f.fold_budget = 20 << 20                                    # the 400-point group needs 15 MiB, a group of <= 128 points 2.2 MiB
        cut = kc.raw_folds(f, groups, R)
        f.fold_budget = None
        again = kc.raw_folds(f, groups, R)
        for a, b, c in zip(whole, cut, again):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a, c)
        f.fold_budget = 1 << 20
        with pytest.raises(ValueError, match=r"group 0 of \d+ points needs"):
            kc.raw_folds(f, groups, R)
        f.fold_budget = None
        np.testing.assert_array_equal(kc.raw_folds(f, groups, R)[0], whole[0])
    finally:
        f.free()


@pytest.mark.parametrize("lay", kc.TRUTH_LAYOUTS)
@pytest.mark.parametrize("name", list(lc.CLASSES))
@pytest.mark.parametrize("n", kc.TRUTH_SIZES)
def test_accuracy_against_long_double(name, n, lay):
    """The device against the long-double brute force from the same float64 factor, with the cpu backend on that factor as the
    yardstick: within 4x its distance, floor 64 * 2^-53, in the norms of kfold_cases.distances.

    Measured 2026-10-19 on an MI355X: all 128 figures inside the bound, the worst (resid of matern52, n = 129, random_sizes) at 0.80
    of it.  The log-determinant carries the first-order correction tr(V P V^T) - g from the gathered columns (DESIGN.md section
    17): without it the factor of the rounded Gram alone gave 2.35e-14 on rbf2d at n = 257 with everything in one group, against
    the cpu backend's 5.4e-15; with it 3.2e-16."""
    L, R, groups, truth = kc.truth_case(name, n, lay)
    c = LooFactor(L, backend="cpu")
    d = LooFactor(L, backend="hip")
    try:
        dc = kc.distances(kc.raw_folds(c, groups, R), truth)
        dd = kc.distances(kc.raw_folds(d, groups, R), truth)
    finally:
        d.free()
    record_parity(f"kfold_{name}_n{n}_{lay}", cond=float(np.linalg.cond(lc.spd(name, n))), **{f"device_{k}": v for k, v in dd.items()},
                  **{f"cpu_{k}": v for k, v in dc.items()})
    print(name, n, lay, "device", dd, "cpu", dc)
    for what in dd:
        assert dd[what] <= max(4 * dc[what], kc.FLOOR), (what, dd[what], dc[what])


def test_model_level():
    n = 129
    K = np.array(lc.spd("matern52", n))
    Y = lc.curves(n, 3, seed=2) + 0.3
    mean = np.full(n, 0.3)
    folds = gm.make_folds(n, 4, "interleaved")
    d = gm.Diagnostic(mean, K, backend="hip")
    try:
        got = d.kfold(Y, folds)
        held = d._loo
        want = gm.kfold_from_factor(d._L.to_host(), Y, folds, mean=mean, backend="hip")
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        d.loo(Y)
        assert d._loo is held and held is not None                  # one resident inverse for both
        np.testing.assert_array_equal(d.kfold(Y[:, 1], folds).mean, got.mean[:, 1])
    finally:
        d.close()
    assert d._loo is None
    t = gm.Diagnostic(mean, K, df=3, backend="hip")
    try:
        with pytest.raises(NotImplementedError, match="Student"):
            t.kfold(Y, folds)
    finally:
        t.close()

    from sklearn.gaussian_process.kernels import Matern
    X = np.arange(n, dtype=float)[:, None]
    kern = Matern(length_scale=4.0, nu=2.5)
    gp = gm.ConjugateGaussianProcess(kern, nugget=1e-8, optimizer=None, backend="hip").fit(X, Y)
    L = np.sqrt(float(np.squeeze(gp.cov_factor_))) * gp._L_dev.to_host()
    want = gm.kfold_from_factor(L, Y, folds, mean=gp.mean(X), backend="hip")
    for g, w in zip(gp.kfold(folds), want):
        np.testing.assert_array_equal(g, w)
    assert gp.kfold(3, y=Y[:, 0]).mean.shape == (n,)
    with pytest.raises(NotImplementedError):
        gm.ConjugateStudentProcess(kern, nugget=1e-8, optimizer=None, backend="hip").fit(X, Y).kfold(3)


def test_refusals_on_the_device():
    """What the library itself refuses, past the Python layer's checks: a fold_ptr that does not start at 0, end at n and increase,
    a fold_idx that is no permutation, bad block indices.  The object works afterwards."""
    from gsum_amd import _loo_lib
    n = 5
    L, W, p = lc.lattice("ones", n)
    f = _loo_lib.DeviceLoo(0, L)
    try:
        R = np.ones((n, 1))
        i64 = lambda *v: np.array(v, dtype=np.int64)                # noqa: E731
        perm = i64(0, 1, 2, 3, 4)
        for ptr, idx, msg in ((i64(1, 5), perm, "start at 0"), (i64(0, 4), perm, "end at n"), (i64(0, 3, 3, 5), perm, "increase strictly"),
                              (i64(0, 6, 5), perm, "increase strictly"), (i64(0, 2, 5), i64(0, 1, 2, 3, 5), "outside 0 ... 4"),
                              (i64(0, 2, 5), i64(0, 1, 2, 3, -1), "outside 0 ... 4"), (i64(0, 2, 5), i64(0, 1, 2, 2, 4), "more than once")):
            with pytest.raises(ValueError, match=msg):
                f.folds(ptr, idx, R)
        with pytest.raises(ValueError, match="n_folds must be <= n"):
            f.folds(i64(0, 1, 2, 3, 4, 5, 5), perm, R)
        with pytest.raises(ValueError):
            f.folds(i64(0, 5), perm, np.ones((4, 1)))
        for idx, msg in ((i64(0, 5), "outside 0 ... 4"), (i64(-1), "outside 0 ... 4"), (i64(1, 1), "more than once"),
                         (i64(0, 1, 2, 3, 4, 0), "g must be <= n")):
            with pytest.raises(ValueError, match=msg):
                f.precision_block(idx)
        resid, var, md2, logdet = f.folds(i64(0, 5), i64(4, 2, 0, 1, 3), R)
        np.testing.assert_allclose(resid, R, rtol=1e-13)
        np.testing.assert_allclose(var, np.arange(1.0, 6.0), rtol=1e-13)                     # K = L L^T has the diagonal 1 .. n
        t = f.fold_times()
        assert set(t) == set(_loo_lib.FOLD_PHASES) and t["gram"] > 0 and t["factor"] > 0
        assert set(f.times()) == set(_loo_lib.PHASES)
    finally:
        f.free()
    with pytest.raises(ValueError):
        f.folds(i64(0, 5), perm, R)                                 # freed


def test_a_block_that_does_not_factor_names_its_group():
    """A NaN below the diagonal: open accepts the factor, kfold raises LinAlgError naming a group, writes nothing and leaves the
    object usable.  A precision that overflows (the cpu test's case) names exactly its group."""
    n = 257
    L, R, _, _ = lc.factor_case("rbf", n)
    Lb = np.array(L)
    Lb[200, 100] = np.nan
    f = LooFactor(Lb, backend="hip")
    try:
        for _ in range(2):
            with pytest.raises(np.linalg.LinAlgError, match=r"group \d+ does not factor.*row \d+"):
                f.folds(R, 5)
        assert f.solve(R).shape == R.shape
        assert f.loo(R).mean.shape == R.shape
    finally:
        f.free()
    g = LooFactor(L, backend="hip")
    try:
        assert np.all(np.isfinite(g.folds(R, 5).mean))
    finally:
        g.free()
    d = np.ones(12)
    d[7] = 1e-200
    h = LooFactor(np.diag(d), backend="hip")
    try:
        with pytest.raises(np.linalg.LinAlgError, match="group 2 does not factor: the pivot of its row 1 "):
            h.folds(np.ones(12), 4)
        np.testing.assert_array_equal(h.precision_block([0, 3]), np.eye(2))
    finally:
        h.free()


def test_outputs_are_untouched_when_a_group_fails():
    from gsum_amd import _loo_lib
    d = np.ones(12)
    d[7] = 1e-200
    f = _loo_lib.DeviceLoo(0, np.diag(d))
    try:
        lib = f._lib
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        ptr, idx, _ = normalise_folds(4, 12)
        R = np.ones((12, 1))
        outs = [np.full(s, -7.0) for s in ((12, 1), 12, (4, 1), 4)]
        rc = lib.gsum_loo_folds(f._h, ptr.ctypes.data_as(ip), idx.ctypes.data_as(ip), 4, R.ctypes.data_as(dp), 1,
                                *[o.ctypes.data_as(dp) for o in outs])
        assert rc != 0 and "group 2 does not factor" in lib.gsum_loo_last_error().decode()
        for o in outs:
            assert np.all(o == -7.0)
    finally:
        f.free()
