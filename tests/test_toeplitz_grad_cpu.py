"""The Toeplitz gradient pieces on backend='cpu' (numpy.longdouble throughout), the host layers on top and the contract of the new entry
points of libgsum_toep.so (no GPU needed).  The shared cases are in toeplitz_grad_cases.py; DESIGN.md section 19."""
import numpy as np
import pytest
from sklearn.gaussian_process.kernels import RBF, ConstantKernel as C, DotProduct, Matern, WhiteKernel

import gsum_amd as gm  # noqa: E402
import toeplitz_cases as tc  # noqa: E402
import toeplitz_grad_cases as gc  # noqa: E402


@pytest.mark.parametrize("n", tc.SIZES)
def test_identities_and_closed_form_inverse_column(n):
    """dt = [t, e_0] on ARFIMA columns: trace(t) = n, H(t) = G, trace(e_0) and x against the closed form, H(e_0) = alpha^T alpha,
    T alpha = Z.  The cpu backend sits within the floor 64 * 2^-53 on all six."""
    gc.check_identities("cpu", n)


def test_closed_form_inverse_column_is_the_inverse():
    """The closed form itself, against numpy's dense inverse of a small well-conditioned case."""
    from scipy.linalg import toeplitz
    for d in tc.DS:
        for n in (1, 2, 5, 40):
            want = np.linalg.inv(toeplitz(tc.arfima_column(n, d)))[:, 0]
            assert np.max(np.abs(gc.arfima_inverse_column(n, d).astype(float) - want)) <= 1e-13 * np.max(np.abs(want))


def test_goldens_cover_the_ill_cases():
    assert gc.golden_names() == [c["name"] for c in sorted(tc.ill_cases(), key=lambda c: (c["n"], c["name"]))]
    assert [c["cols"] for c in gc.golden()["cases"] if c["n"] == 4097] == [2]


@pytest.mark.parametrize("name", tc.ill_names())
def test_ill_conditioned_goldens(name):
    gc.check_golden("cpu", name)


def test_properties():
    gc.check_properties("cpu")


def test_a_failing_first_column_between_two_good_ones():
    gc.check_failure_between_good("cpu")


def test_shape_refusals():
    gc.check_shape_refusals("cpu")


def test_library_refuses_bad_arguments_before_it_touches_a_device():
    """Null pointers, n above the limit, P < 1 and t[0] outside 2^-64 .. 2^64, on a null handle or none: no device is opened."""
    import ctypes as C_
    from gsum_amd import _toep_lib
    from gsum_amd._sidelib import _d, _i32
    lib = _toep_lib.load_library()
    err = lambda: lib.gsum_toep_last_error().decode()  # noqa: E731
    assert lib.gsum_toep_grad(None, None, 1, 1, None, 1, None, 1, 1, None, None, None, None, None) != 0 and "null pointer" in err()
    assert lib.gsum_toep_solve(None, None, 1, 1, None, 1, None, None, None) != 0 and "null pointer" in err()
    assert lib.gsum_toep_grad_times(None, None, 0) != 0 and "null pointer" in err()
    fake = C_.c_void_p(1)                                               # never dereferenced: every refusal comes first
    n = 8193
    t, Z, info = np.ones(n), np.ones(n), np.zeros(1, dtype=np.int32)
    out = np.zeros(n)
    assert lib.gsum_toep_grad(fake, _d(t), 1, n, _d(t), 1, _d(Z), 1, 1, _d(out), _d(out), _i32(info), _d(out), _d(out)) != 0
    assert "n must be <= 8192" in err()
    assert lib.gsum_toep_solve(fake, _d(t), 1, n, _d(Z), 1, _d(out), None, _i32(info)) != 0 and "n must be <= 8192" in err()
    t8 = tc.kms_column(8, 0.5)
    assert lib.gsum_toep_grad(fake, _d(t8), 1, 8, _d(t8), 0, _d(Z), 1, 1, _d(out), _d(out), _i32(info), _d(out), _d(out)) != 0
    assert "P must be" in err()
    for s in (2.0 ** -66, 2.0 ** 66):
        ts = s * t8
        assert lib.gsum_toep_grad(fake, _d(ts), 1, 8, _d(t8), 1, _d(Z), 1, 1, _d(out), _d(out), _i32(info), _d(out), _d(out)) != 0
        assert "t[0] must lie within" in err()
        assert lib.gsum_toep_solve(fake, _d(ts), 1, 8, None, 0, _d(out), None, _i32(info)) != 0 and "t[0] must lie within" in err()
    assert _toep_lib.GRAD_PHASES == ("h2d", "schur", "levinson", "gram", "diagsums", "solve", "contract", "d2h")
    assert _toep_lib.PHASES == ("h2d", "schur", "gram", "d2h")
    for name in ("toeplitz_inverse_column", "toeplitz_solve", "toeplitz_grad", "toeplitz_gradient_columns"):
        assert name in gm.__all__ and hasattr(gm, name)


KERNELS = [RBF(0.2), Matern(0.3, nu=0.5), Matern(0.3, nu=1.5), Matern(0.3, nu=2.5), C(2.0) * RBF(0.2) + WhiteKernel(1e-3),
           C(2.0, "fixed") * RBF(0.2, "fixed") + WhiteKernel(1e-3, "fixed")]


@pytest.mark.parametrize("kernel", KERNELS, ids=str)
def test_gradient_columns_are_column_zero_of_the_dense_gradient(kernel):
    """n = 300: the block loop runs more than once.  Bit for bit, at the kernel's own theta and at another."""
    X = np.linspace(0, 1, 300)[:, None]
    want = kernel(X, eval_gradient=True)[1][:, 0, :].T
    got = gm.toeplitz_gradient_columns(kernel, X)
    assert got.shape == (kernel.n_dims, 300) and np.array_equal(got, want)
    assert np.array_equal(gm.toeplitz_gradient_columns(kernel, X[:, 0]), want)
    if kernel.n_dims:
        theta = kernel.theta + 0.3
        assert np.array_equal(gm.toeplitz_gradient_columns(kernel, X, theta), kernel.clone_with_theta(theta)(X, eval_gradient=True)[1][:, 0, :].T)
        assert np.array_equal(kernel.theta, KERNELS[[str(k) for k in KERNELS].index(str(kernel))].theta)          # the caller's kernel is not touched
    else:
        assert got.shape == (0, 300)


def test_gradient_columns_diagonal_and_refusals():
    X = np.linspace(0, 1, 9)[:, None]
    k = C(2.0) * RBF(0.2) + WhiteKernel(1e-3)
    dt = gm.toeplitz_gradient_columns(k, X)
    assert dt[2, 0] == 1e-3 and np.all(dt[2, 1:] == 0)                 # a free WhiteKernel: its noise level on the diagonal alone
    assert dt[0, 0] == 2.0 and dt[1, 0] == 0.0                         # the constant's derivative is the kernel value; a length scale's is 0 at distance 0
    with pytest.raises(NotImplementedError, match="stationary"):
        gm.toeplitz_gradient_columns(RBF(0.2) * DotProduct(1.0), X)
    with pytest.raises(ValueError, match="one feature"):
        gm.toeplitz_gradient_columns(RBF(0.2), np.zeros((9, 2)))


@pytest.mark.parametrize("name", [c[0] for c in gc.MODEL_CLASSES])
def test_model_gradient_against_long_double_truth(name):
    gc.check_model_gradient("cpu", name, 40)


@pytest.mark.parametrize("name", [c[0] for c in gc.MODEL_CLASSES])
def test_fit_on_the_structured_route(name, monkeypatch):
    """Achieved |structured - dense| / |dense| of the optimum's value on backend='cpu' at n = 40: 0 for both classes (bound 2.2e-7)."""
    gc.check_fit("cpu", name, 40, monkeypatch)


def test_model_layer_refusals_and_failures():
    X, y = gc.model_xy(40)
    gp = gc.model_process(gm.ConjugateGaussianProcess, "cpu", optimizer=None)
    th = np.log([0.1])
    with pytest.raises(ValueError, match="structure"):
        gp.log_marginal_likelihood_batch([th], X=X, y=y, structure="circulant", eval_gradient=True)
    with pytest.raises(NotImplementedError, match="gradient"):         # the single call keeps its refusal; the batch is the gradient's entry
        gp.log_marginal_likelihood(th, eval_gradient=True, X=X, y=y, structure="toeplitz")
    Xj = X.copy()
    Xj[7] += 1e-9
    for bad in (dict(X=Xj), dict(X=np.random.RandomState(0).rand(40, 2))):
        with pytest.raises(ValueError):
            gp.log_marginal_likelihood_batch([th], y=y, structure="toeplitz", eval_gradient=True, **bad)
        with pytest.raises(ValueError):
            gc.model_process(gm.ConjugateGaussianProcess, "cpu").fit(bad["X"], y, structure="toeplitz")
    with pytest.raises(ValueError, match="structure"):
        gc.model_process(gm.ConjugateGaussianProcess, "cpu").fit(X, y, structure="circulant")
    dot = gm.ConjugateGaussianProcess(kernel=RBF(0.2) * DotProduct(1.0), backend="cpu")
    with pytest.raises(NotImplementedError, match="stationary"):
        dot.fit(X, y, structure="toeplitz")
    # a matrix that does not factor: (-inf, zeros), as on the dense route
    flat = gm.ConjugateGaussianProcess(kernel=RBF(0.2), optimizer=None, nugget=0.0, backend="cpu")
    got = flat.log_marginal_likelihood_batch([np.log([1e12]), np.log([0.05])], X=X, y=y, structure="toeplitz", eval_gradient=True)
    assert got[0][0] == -np.inf and np.array_equal(got[0][1], np.zeros(1)) and np.isfinite(got[1][0]) and np.isfinite(got[1][1]).all()
    # no free hyperparameter: the values with empty gradients
    fixed = gm.ConjugateGaussianProcess(kernel=RBF(0.2, "fixed"), optimizer=None, backend="cpu")
    got = fixed.log_marginal_likelihood_batch([np.zeros(0)], X=X, y=y, structure="toeplitz", eval_gradient=True)
    assert got[0][1].shape == (0,) and got[0][0] == fixed.log_marginal_likelihood_batch([np.zeros(0)], X=X, y=y, structure="toeplitz")[0]


def test_truncation_fit_on_the_structured_route(monkeypatch):
    """TruncationGP.fit(structure="toeplitz") and TruncationTP's, inherited: the coefficients' process calibrates on the structured
    route and ends at the dense fit's optimum."""
    X, c = gc.model_xy(40)
    orders = np.arange(3)
    y = gm.partials(c, ratio=0.5, ref=1.0, orders=orders)
    for cls in (gm.TruncationGP, gm.TruncationTP):
        kw = dict(kernel=Matern(0.2, nu=0.5) + WhiteKernel(1e-6, noise_level_bounds="fixed"), ratio=0.5, ref=1.0, backend="cpu")
        dense = cls(**kw).fit(X, y, orders=orders)
        tg = cls(**kw)
        with monkeypatch.context() as mpc:
            cnt = gc.Counters(mpc, tg.coeffs_process)
            tg.fit(X, y, orders=orders, structure="toeplitz")
            assert cnt.structured > 0 and cnt.dense == 0
        v_s, v_d = tg.coeffs_process.log_marginal_likelihood_value_, dense.coeffs_process.log_marginal_likelihood_value_
        assert abs(v_s - v_d) <= 100 * gc.FACTR_EPS * abs(v_d)
