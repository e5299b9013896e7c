"""The Toeplitz likelihood path on backend='cpu' (the recursion with a numpy.longdouble generator), its host layers, and the contract of
libgsum_toep.so (no GPU needed).  The shared cases are in toeplitz_cases.py."""
import os
import re
import subprocess

import numpy as np
import pytest
from sklearn.gaussian_process.kernels import RBF, DotProduct, Matern, WhiteKernel

from conftest import ROOT

import gsum_amd as gm  # noqa: E402
import toeplitz_cases as tc  # noqa: E402
from toeplitz_cases import notebook_process  # noqa: E402


@pytest.mark.parametrize("n", tc.SIZES)
def test_closed_form_sizes(n):
    tc.check_closed_form("cpu", n)


@pytest.mark.parametrize("n,c,n_sets,m", tc.SHAPES)
def test_closed_form_shapes(n, c, n_sets, m):
    tc.check_closed_form("cpu", n, c, n_sets, m)


def test_failures():
    tc.check_failures("cpu")


def test_properties():
    tc.check_properties("cpu")


@pytest.mark.parametrize("name", tc.ill_names())
def test_ill_conditioned_goldens(name):
    tc.check_ill("cpu", name)


@pytest.mark.parametrize("n", [n for n in tc.SIZES if n >= 3])
def test_arfima_sizes(n):
    """ARFIMA(0, d, 0), d over (0.4, -0.3): every step of the recursion rotates.  sum_log_diag within the floor of the closed form (so
    rounding t to fp64 does not move the answer); G within the rule of the mpmath golden at n = 513, 2049, 4097 and 8192."""
    tc.check_arfima("cpu", n)


def test_arfima_goldens_cover_the_upper_classes_and_the_limit():
    assert tc.arfima_golden_sizes() == [513, 2049, 4097, 8192]
    assert [c["n"] for c in tc.classes_golden()["ill"]] == [513, 2049, 4097]
    assert os.path.getsize(tc.CLASSES_GOLDEN) < 473 * 1024


def test_arfima_reflection_coefficients_never_vanish():
    """What makes the family a test of the rotation: the coefficients of the cpu recursion's own column are d / (k - d), none zero; the
    Kac-Murdock-Szego column's are [rho, 0, 0, ...], so after its first step v is zero and a step only shifts u."""
    def coefficients(t):
        u = np.asarray(t, dtype=tc.LD) / np.sqrt(tc.LD(t[0]))
        v = u.copy()
        v[0] = 0
        out = []
        for k in range(len(t) - 1):
            rho = v[k + 1] / u[k]
            out.append(float(rho))
            ic = 1 / np.sqrt((1 - rho) * (1 + rho))
            us, vv = u[k:-1].copy(), v[k + 1:].copy()
            u[k + 1:], v[k + 1:] = (us - rho * vv) * ic, (vv - rho * us) * ic
        return np.array(out)
    n = 200
    for d in tc.DS + (0.25,):
        g = coefficients(tc.arfima_column(n, d))
        assert np.max(np.abs(g - d / (np.arange(1, n) - d))) <= 4e-16 and np.min(np.abs(g)) > 1e-3
        E = tc.arfima_energies(n, d)
        assert np.allclose(np.cumprod(1 - g ** 2), np.asarray(E[1:], dtype=float), rtol=1e-13, atol=0)
    g = coefficients(tc.kms_column(n, 0.5))
    assert g[0] == 0.5 and np.max(np.abs(g[1:])) == 0.0


@pytest.mark.parametrize("n", tc.LATE_SIZES)
def test_late_failures(n):
    ps, p_nan = tc.late_positions(n)
    info = tc.check_late_failures("cpu", n)
    assert sorted(info) == sorted([0] + [p + 1 for p in ps] + [p_nan + 1]) and len(set(ps)) == len(ps)


def test_chunked_shape_arithmetic():
    """The shape of the device test of the first-column loop, in the library's arithmetic (gsum_toep.hip): one first column per launch,
    so three launches; one set fewer and two would fit; every other shape of the suite goes through in one launch."""
    s = tc.CHUNKED
    ncols = s["n_sets"] * s["c"]
    assert tc.first_columns_per_launch(s["n"], ncols, s["m"]) == 1
    assert tc.first_columns_per_launch(s["n"], ncols - s["c"], s["m"]) == 2
    assert s["n"] * ncols < 2 ** 31 and s["n_sets"] <= 65535
    assert 128 << 20 < s["n"] * ncols * 8 < 130 << 20
    for n, c, n_sets, m in tc.SHAPES:
        assert tc.first_columns_per_launch(n, c * n_sets, m) == m
    src = open(os.path.join(ROOT, "gsum_amd", "csrc", "gsum_toep.hip")).read()
    assert "kYBudget = (size_t)256 << 20" in src and tc.Y_BUDGET == 256 << 20


def test_scaling():
    tc.check_scaling("cpu")


@pytest.mark.parametrize("a", tc.FAR)
def test_far_scaling(a):
    tc.check_far_scaling("cpu", a)


def test_uniform_grid_step():
    for scale in (1.0, 3.7, 1e-3, 123456.789):
        for n in (2, 5, 100, 8192):
            X = scale * np.linspace(0, 1, n)
            assert gm.uniform_grid_step(X[:, None]) == pytest.approx(scale / (n - 1), rel=1e-14)
    assert gm.uniform_grid_step(0.1 * np.arange(8192)) == pytest.approx(0.1, rel=1e-14)
    assert gm.uniform_grid_step(np.linspace(0, 1, 100)[1::24]) == pytest.approx(24 / 99, rel=1e-14)
    assert gm.uniform_grid_step(np.array([[0.3]])) == 0.0                                   # one point
    assert gm.uniform_grid_step(np.linspace(2, -1, 31)) == pytest.approx(-0.1, rel=1e-14)   # a decreasing grid
    X = np.linspace(0, 1, 101)
    X[40] += 16 * np.finfo(float).eps * np.max(np.abs(X))
    with pytest.raises(ValueError, match="index 40"):
        gm.uniform_grid_step(X)
    X = np.linspace(0, 1, 11)
    X[5] = X[4]
    with pytest.raises(ValueError, match="index 5"):
        gm.uniform_grid_step(X)
    with pytest.raises(ValueError, match="one feature"):
        gm.uniform_grid_step(np.zeros((4, 2)))


@pytest.mark.parametrize("kernel", [RBF(0.2), Matern(0.3, nu=2.5), Matern(0.3, nu=0.5), 2.0 * RBF(0.2) + WhiteKernel(1e-3)], ids=str)
def test_toeplitz_column_is_the_dense_first_column(kernel):
    X = np.linspace(0, 1, 97)[:, None]
    from gsum_amd._cpu import cpu_context
    K = cpu_context().kernel_matrix(gm.describe_kernel(kernel, 1), X)
    want = K[:, 0].copy()
    want[0] += 1e-10
    assert np.array_equal(gm.toeplitz_column(kernel, X, 1e-10, backend="cpu"), want)
    assert np.array_equal(gm.toeplitz_column(kernel, X[:, 0], 1e-10, backend="cpu"), want)


def test_toeplitz_column_refusals():
    X = np.linspace(0, 1, 9)[:, None]
    with pytest.raises(NotImplementedError, match="stationary"):
        gm.toeplitz_column(RBF(0.2) * DotProduct(1.0), X, backend="cpu")
    with pytest.raises(ValueError, match="one feature"):
        gm.toeplitz_column(RBF(0.2), np.zeros((9, 2)), backend="cpu")
    with pytest.raises(ValueError, match="at most 16"):
        gm.toeplitz_gram(np.ones(4), np.ones((4, 17)), backend="cpu")
    with pytest.raises(ValueError, match="n_sets"):
        gm.toeplitz_gram(np.ones(4), np.ones((4, 5)), n_sets=2, backend="cpu")


def test_exports_and_library_contract():
    """include/gsum_toep.h is the contract of libgsum_toep.so: every function it declares is exported and bound, nothing else."""
    from gsum_amd import _toep_lib, build
    for name in ("uniform_grid_step", "toeplitz_column", "toeplitz_gram"):
        assert name in gm.__all__ and hasattr(gm, name)
    assert "toep" in build.SIDE
    header = open(os.path.join(ROOT, "include", "gsum_toep.h")).read()
    declared = set(re.findall(r"\b(gsum_toep_[a-z0-9_]+)\s*\(", header))
    assert declared and declared == set(_toep_lib.PROTOTYPES), declared ^ set(_toep_lib.PROTOTYPES)
    path = build.build_toep()
    assert path == _toep_lib.LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("gsum_")}
    assert exported == declared
    assert _toep_lib.max_n() == 8192                                                       # needs no device


def test_library_refuses_bad_arguments_before_it_touches_a_device():
    import ctypes as C
    from gsum_amd import _toep_lib
    lib = _toep_lib.load_library()
    assert lib.gsum_toep_gram(None, None, 1, 1, None, 1, 1, None, None, None) != 0
    assert "null pointer" in lib.gsum_toep_last_error().decode()
    assert lib.gsum_toep_open(0, None) != 0 and "null pointer" in lib.gsum_toep_last_error().decode()
    lib.gsum_toep_close(None)


def _process(cls=None, **kw):
    cls = cls or gm.ConjugateGaussianProcess
    # Matern-1/2 is well conditioned (cond(R) in the hundreds here): the Toeplitz defect of kernel(X) times it stays far below 1e-12
    return cls(kernel=Matern(0.2, nu=0.5) + WhiteKernel(1e-6, noise_level_bounds="fixed"), optimizer=None, backend="cpu", **kw)


def _xy(n=40, r=3):
    X = np.linspace(0, 1, n)[:, None]
    return X, np.random.RandomState(1).randn(n, r)


def test_process_likelihood_matches_the_dense_route():
    X, y = _xy()
    thetas = [np.log([0.05]), np.log([0.1]), np.log([0.15])]
    for cls, kw in ((gm.ConjugateGaussianProcess, dict(center=0.1, disp=1.5, df=2, scale=0.7)), (gm.ConjugateStudentProcess, dict(df=3, scale=0.9))):
        gp = _process(cls, **kw)
        dense = [gp.log_marginal_likelihood(t, X=X, y=y) for t in thetas]
        one = [gp.log_marginal_likelihood(t, X=X, y=y, structure="toeplitz") for t in thetas]
        batch = gp.log_marginal_likelihood_batch(thetas, X=X, y=y, structure="toeplitz")
        np.testing.assert_allclose(one, dense, rtol=1e-12)
        assert np.array_equal(batch, one)
    gp.fit(X, y)
    assert gp.log_marginal_likelihood(structure="toeplitz") == pytest.approx(gp.log_marginal_likelihood(), rel=1e-12)


def test_refusals_of_the_model_layer():
    X, y = _xy()
    gp = _process()
    th = np.log([0.1])
    with pytest.raises(ValueError, match="structure"):
        gp.log_marginal_likelihood(th, X=X, y=y, structure="circulant")
    with pytest.raises(ValueError, match="structure"):
        gp.log_marginal_likelihood_batch([th], X=X, y=y, structure="dense")
    with pytest.raises(NotImplementedError, match="gradient"):
        gp.log_marginal_likelihood(th, eval_gradient=True, X=X, y=y, structure="toeplitz")
    with pytest.raises(ValueError, match="at most 15 curves"):
        gp.log_marginal_likelihood(th, X=X, y=np.ones((40, 16)), structure="toeplitz")
    Xj = X.copy()
    Xj[7] += 1e-9
    with pytest.raises(ValueError, match="index 7"):
        gp.log_marginal_likelihood(th, X=Xj, y=y, structure="toeplitz")
    with pytest.raises(ValueError, match=r"\(n, 1\)"):
        gp.log_marginal_likelihood(th, X=np.random.RandomState(0).rand(40, 2), y=y, structure="toeplitz")
    dot = gm.ConjugateGaussianProcess(kernel=RBF(0.2) * DotProduct(1.0), optimizer=None, backend="cpu")
    with pytest.raises(NotImplementedError, match="stationary"):
        dot.log_marginal_likelihood(None, X=X, y=y, structure="toeplitz")
    tg = gm.TruncationGP(kernel=RBF(0.2), ratio=0.5, ref=1.0, optimizer=None, backend="cpu")
    tg.fit(X, gm.partials(y, ratio=0.5, ref=1.0, orders=np.arange(3)), orders=np.arange(3))
    for kw in (dict(structure="circulant"), dict(structure="toeplitz", devices="all"), dict(structure="toeplitz", gather="rccl"),
               dict(structure="toeplitz", mode="fast"), dict(structure="toeplitz", X=Xj)):
        with pytest.raises(ValueError):
            tg.log_marginal_likelihood_grid([th], [0.4, 0.5], **kw)
    big = gm.TruncationGP(kernel=RBF(0.2), ratio=0.5, ref=1.0, optimizer=None, backend="cpu")
    big.fit(X, np.cumsum(np.random.RandomState(2).randn(40, 17), axis=1), orders=np.arange(17))
    with pytest.raises(ValueError, match="at most 15 curves"):
        big.log_marginal_likelihood_grid([th], [0.5], structure="toeplitz")


def test_a_matrix_that_does_not_factor_is_minus_infinity():
    """RBF with a length scale of 1e12 and no nugget: t is all ones, info 2, -inf as on the dense route (models.py:970-972)."""
    X, y = _xy()
    gp = gm.ConjugateGaussianProcess(kernel=RBF(0.2), optimizer=None, nugget=0.0, backend="cpu")
    thetas = [np.log([1e12]), np.log([0.05])]
    got = gp.log_marginal_likelihood_batch(thetas, X=X, y=y, structure="toeplitz")
    assert got[0] == -np.inf and np.isfinite(got[1])
    assert gp.log_marginal_likelihood(thetas[0], X=X, y=y, structure="toeplitz") == -np.inf
    tg = gm.TruncationGP(kernel=RBF(0.2), ratio=0.5, ref=1.0, optimizer=None, nugget=0.0, backend="cpu")
    tg.X_train_, tg.y_train_, tg.orders_ = X, gm.partials(y, ratio=0.5, ref=1.0, orders=np.arange(3)), np.arange(3)
    grid = tg.log_marginal_likelihood_grid(thetas, [0.4, 0.5], structure="toeplitz")
    assert np.all(grid[:, 0] == -np.inf) and np.all(np.isfinite(grid[:, 1]))


def test_notebook_grid_known_answer(notebook_grid):
    """The reference's recorded 80 x 100 (Q, ell) scan through the structured path: argmax (36, 39) and every entry at rtol 1e-12
    (the numpy model of the recursion measured 1.8e-14)."""
    g = notebook_grid
    gp, thetas = notebook_process(g, gm.TruncationGP, "cpu")
    want = np.array(g["grid"])
    grids = [gp.log_marginal_likelihood_grid(thetas, g["ratio_vals"], mode=mode, structure="toeplitz") for mode in ("full", "reuse")]
    assert np.array_equal(grids[0], grids[1])
    grid = grids[0]
    assert list(np.unravel_index(np.argmax(grid), grid.shape)) == [36, 39]
    assert not np.isneginf(grid).any() and not np.isnan(grid).any()
    print("toeplitz notebook grid cpu: max rel", float(np.max(np.abs(grid - want) / np.abs(want))))
    np.testing.assert_allclose(grid, want, rtol=1e-12)


def test_grid_against_the_dense_route(notebook_grid):
    """With and without ``scales``, the Student class, and shards of whole thetas: the dense cpu route on the same inputs, rtol 1e-12."""
    g = notebook_grid
    ratios = g["ratio_vals"][::9]
    gp, thetas = notebook_process(g, gm.TruncationGP, "cpu")
    thetas = thetas[::7]
    dense = gp.log_marginal_likelihood_grid(thetas, ratios)
    got = gp.log_marginal_likelihood_grid(thetas, ratios, structure="toeplitz")
    np.testing.assert_allclose(got, dense, rtol=1e-12)
    scales = [0.5, 1.0, 2.5]
    np.testing.assert_allclose(gp.log_marginal_likelihood_grid(thetas, ratios, scales=scales, structure="toeplitz"),
                               gp.log_marginal_likelihood_grid(thetas, ratios, scales=scales), rtol=1e-12)
    merged = np.full_like(got, np.nan)
    for rank in range(4):
        part = gp.log_marginal_likelihood_grid(thetas, ratios, structure="toeplitz", shard=(rank, 4))
        own = ~np.isnan(part)
        assert np.all(own == own[0]) and not np.any(own & ~np.isnan(merged))               # whole thetas, each owned once
        merged[own] = part[own]
    assert np.array_equal(merged, got)
    tp, _ = notebook_process(g, gm.TruncationTP, "cpu")
    np.testing.assert_allclose(tp.log_marginal_likelihood_grid(thetas, ratios, structure="toeplitz"),
                               tp.log_marginal_likelihood_grid(thetas, ratios), rtol=1e-12)
