"""The non-finite and degenerate-input contract without a GPU: every expectation of tests/nonfinite_cases.py is
proved here against scikit-learn's matrix and netlib's unblocked dpotf2 in plain numpy, and ``backend="cpu"`` is held to it -- the
same info as the device for a NaN in the data (``CpuContext.potrf``: the optimised LAPACK returns info 0 and a NaN factor there), the
same refusals from ``describe_kernel``, and the closed-form pieces inside the derived bounds that the device tests then use."""
from __future__ import annotations

import numpy as np
import pytest
from sklearn.gaussian_process.kernels import RBF, ConstantKernel as C, Matern, WhiteKernel

import nonfinite_cases as nc
from gsum_amd.kernels import describe_gradient, describe_kernel
from gsum_amd._cpu import CpuContext

ALL_ORDERS = nc.ONE_WORKGROUP + nc.MEDIUM + nc.LARGE


@pytest.fixture()
def cpu():
    return CpuContext()


def _desc(kernel):
    return describe_kernel(kernel, 1)


# ---- netlib's rule and the expectations ------------------------------------------------------------------------------------------------
def test_dpotf2_is_cholesky_on_a_clean_matrix():
    A = nc.sk_matrix(nc.dense(), nc.grid(60))
    L, info = nc.dpotf2(A)
    assert info == 0
    assert not np.any(np.triu(L, 1))
    assert np.all(np.abs(L @ L.T - A) <= 2 * 61 * nc.EPS * (np.abs(L) @ np.abs(L).T))        # (Higham, Theorem 10.3: (n + 1) eps |L| |L|^T)
    A[40, 40] = -1.0
    assert nc.dpotf2(A)[1] == 41
    assert nc.dpotf2(np.diag(np.r_[np.ones(3), 0.0, 1.0]))[1] == 4
    assert nc.dpotf2(np.diag(np.r_[np.ones(3), np.nan, 1.0]))[1] == 4
    B = np.eye(5)
    B[0, 3] = np.nan                                                   # (the strict upper triangle is never read)
    assert nc.dpotf2(B)[1] == 0


@pytest.mark.parametrize("name", list(nc.KERNELS))
def test_clean_matrices_factor(cpu, name):
    for n in ALL_ORDERS:
        assert nc.clean_info(name, n) == 0
        assert cpu.lml_batch([_desc(nc.KERNELS[name]())], nc.grid(n), nc.rhs(n), nc.NUGGET)[2][0] == 0


@pytest.mark.parametrize("n", ALL_ORDERS)
@pytest.mark.parametrize("name", list(nc.KERNELS))
def test_nan_point_info(cpu, name, n):
    """X[i] = NaN: scikit-learn's matrix is NaN in row and column i off a finite diagonal; netlib's rule gives info_of_nan_point on it,
    and backend="cpu" returns the same (the parent returned 0: LAPACK's own info)."""
    kernel = nc.KERNELS[name]()
    desc = _desc(kernel)
    for i in nc.plant_rows(n):
        X = nc.plant_point(nc.grid(n), i)
        K = nc.sk_matrix(kernel, X)
        off = ~np.eye(n, dtype=bool)
        assert np.all(np.isfinite(np.diag(K)))
        assert np.all(np.isnan(K[i][off[i]])) and np.all(np.isnan(K[:, i][off[:, i]]))
        assert np.all(np.isfinite(np.delete(np.delete(K, i, 0), i, 1)))
        want = nc.info_of_nan_point(n, i)
        assert nc.dpotf2(K)[1] == want
        G, sld, info = cpu.lml_batch([desc], X, nc.rhs(n), nc.NUGGET)
        assert info[0] == want


@pytest.mark.parametrize("n", (2, 17, 300))
def test_cpu_potrf_applies_netlibs_nan_test(cpu, n):
    """The fix itself, on an uploaded matrix: info is the first NaN pivot, the matrix is consumed as for any info > 0, and what follows
    a failed factorisation follows: sqrt_errors raises, the gradient's pieces are zeros."""
    for i in sorted({0, n // 2, n - 1}):
        X = nc.plant_point(nc.grid(n), i)
        want = nc.info_of_nan_point(n, i)
        for kernel in (C(2.0) * RBF(0.3) + WhiteKernel(1e-3), Matern(0.7, nu=1.5) + WhiteKernel(1e-3)):
            K = nc.sk_matrix(kernel, X, 0.0)
            M = cpu.upload(K)
            assert cpu.potrf(M) == want
            assert M.failed and not M.factored
            with pytest.raises(ValueError, match="failed factorisation"):
                cpu.forward_gram(M, nc.rhs(n))
            with pytest.raises(np.linalg.LinAlgError):
                cpu.sqrt_errors(cpu.upload(K), nc.rhs(n))
            info_p, _ = cpu.pstrf(cpu.upload(K))
            assert info_p > 0                                           # (LAPACK's dpstrf stops on a NaN by itself: section 11)
            params = describe_gradient(kernel, 1)
            G, sld, info, trace, H = cpu.lml_grad(_desc(kernel), params, X, nc.rhs(n), 0.0)
            assert info == want
            assert not np.any(trace) and not np.any(H)


def test_cpu_potrf_clean_and_ordinary_failures_unchanged(cpu):
    A = nc.sk_matrix(nc.dense(), nc.grid(50))
    M = cpu.upload(A)
    assert cpu.potrf(M) == 0 and M.factored and not M.failed
    np.testing.assert_array_equal(M.to_host(), np.tril(np.linalg.cholesky(A)))
    A[30, 30] = -1.0
    M = cpu.upload(A)
    assert cpu.potrf(M) == 31 and M.failed


@pytest.mark.parametrize("n", (2, 17, 129, 385))
def test_infinite_point_is_family_dependent(cpu, n):
    """X[i] = +-inf.  RBF: exp(-inf) = 0, row i is exactly zero off the diagonal -- a valid matrix, info 0.  Matern-3/2:
    (1 + inf) * exp(-inf) = inf * 0 = NaN, the NaN point's info."""
    for value in (np.inf, -np.inf):
        for i in sorted({0, n // 2, n - 1}):
            X = nc.plant_point(nc.grid(n), i, value)
            K = nc.sk_matrix(nc.banded(), X)
            off = ~np.eye(n, dtype=bool)
            assert np.all(K[i][off[i]] == 0.0) and np.all(K[:, i][off[:, i]] == 0.0)
            assert nc.dpotf2(K)[1] == 0
            assert cpu.lml_batch([_desc(nc.banded())], X, nc.rhs(n), nc.NUGGET)[2][0] == 0
            K = nc.sk_matrix(nc.dense(), X)
            assert np.all(np.isnan(K[i][off[i]]))
            want = nc.info_of_nan_point(n, i)
            assert nc.dpotf2(K)[1] == want
            assert cpu.lml_batch([_desc(nc.dense())], X, nc.rhs(n), nc.NUGGET)[2][0] == want


# ---- hyperparameters at the end of an optimiser's walk ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ls", nc.REFUSED_LENGTH_SCALES)
def test_length_scales_refused_by_the_binding(ls):
    """0, negative and NaN: one ValueError that names the parameter, from describe_kernel and describe_gradient, so for every backend
    alike (the device library itself refuses such a descriptor; scikit-learn would build a matrix that is NaN off the diagonal)."""
    flat = C(1.0) * RBF(1.0) + WhiteKernel(1e-3)
    flat.k1.k2.length_scale = ls
    two = C(1.0) * RBF(1.0) + Matern(1.0, nu=1.5)
    two.k2.length_scale = ls
    for kernel in (flat, two):
        with pytest.raises(ValueError, match="length_scale"):
            describe_kernel(kernel, 1)
        with pytest.raises(ValueError, match="length_scale"):
            describe_gradient(kernel, 1)
    aniso = RBF([1.0, 1.0])
    aniso.length_scale = np.array([1.0, ls])
    with pytest.raises(ValueError, match="length_scale"):
        describe_kernel(aniso, 2)


def test_huge_and_infinite_length_scales_pass():
    for ls in (1e300, np.inf):
        assert describe_kernel(RBF(ls), 1).length_scale[0] == ls


@pytest.mark.parametrize("n", (2, 17, 129, 385))
def test_bad_members_info(cpu, n):
    """The all-ones matrix fails at pivot 1 (1 - 1 = 0 exactly), the zero matrix at pivot 0, by netlib's rule and on backend="cpu"."""
    for name, (kernel, want) in nc.bad_members().items():
        K = nc.sk_matrix(kernel, nc.grid(n), 0.0)
        if name.startswith("ls"):
            assert np.all(K == 1.0)
        else:
            assert not np.any(K)
        assert nc.dpotf2(K)[1] == want
        assert cpu.lml_batch([_desc(kernel)], nc.grid(n), nc.rhs(n), 0.0)[2][0] == want


@pytest.mark.parametrize("m", nc.BATCHES)
def test_batch_members_are_independent_cpu(cpu, m):
    n = 129
    X, Z = nc.grid(n), nc.rhs(n)
    good = [_desc(nc.healthy(ls)) for ls in nc.batch_length_scales(m)]
    want = cpu.lml_batch(good, X, Z, 0.0)
    assert not np.any(want[2])
    for name, (kernel, info_bad) in nc.bad_members().items():
        for pos in nc.bad_positions(m):
            descs = list(good)
            descs[pos] = _desc(kernel)
            G, sld, info = cpu.lml_batch(descs, X, Z, 0.0)
            keep = np.arange(m) != pos
            assert info[pos] == info_bad
            np.testing.assert_array_equal(info[keep], want[2][keep])
            np.testing.assert_array_equal(sld[keep], want[1][keep])
            np.testing.assert_array_equal(G[keep], want[0][keep])


# ---- non-finite right-hand sides -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (17, 129))
@pytest.mark.parametrize("name", ("banded", "dense"))
def test_nonfinite_rhs_expectations(cpu, name, n):
    """What a planted Z[r, c] does in the reference arithmetic (forward substitution on the Cholesky factor, then W^T W): info and
    sum log L_ii do not read Z, column c of W is non-finite from row r on and untouched above it, every G[a, b] with a, b != c keeps
    its bits, row and column c of G are non-finite throughout.  backend="cpu" itself REFUSES such right-hand sides: scipy's
    triangular solve checks its operands ("array must not contain infs or NaNs"), a ValueError as for any other bad argument."""
    from scipy.linalg import solve_triangular
    kernel = nc.KERNELS[name]()
    X, Z = nc.grid(n), nc.rhs(n)
    L, info = nc.dpotf2(nc.sk_matrix(kernel, X))
    assert info == 0
    W0 = solve_triangular(L, Z, lower=True)
    G0 = W0.T @ W0
    k = Z.shape[1]
    for value in nc.NONFINITE:
        for r in (0, n // 2, n - 1):
            for c in (0, k - 1):
                Zp = nc.plant_rhs(Z, r, c, value)
                with np.errstate(all="ignore"):
                    W = solve_triangular(L, Zp, lower=True, check_finite=False)
                    G = W.T @ W
                keep = np.arange(k) != c
                np.testing.assert_array_equal(W[:, keep], W0[:, keep])
                np.testing.assert_array_equal(W[:r, c], W0[:r, c])
                assert not np.any(np.isfinite(W[r:, c]))
                np.testing.assert_array_equal(G[np.ix_(keep, keep)], G0[np.ix_(keep, keep)])
                assert not np.any(np.isfinite(G[c])) and not np.any(np.isfinite(G[:, c]))
                with pytest.raises(ValueError, match="infs or NaNs"):
                    cpu.lml_batch([_desc(kernel)], X, Zp, nc.NUGGET)


# ---- the closed form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", (nc.CLOSED_A, 0.0))
@pytest.mark.parametrize("n", ALL_ORDERS)
def test_closed_form_reference_inside_the_bounds(cpu, n, a):
    """scikit-learn's matrix IS s I with s = closed_scale, and the float64 reference stays inside the derived bounds of closed_form:
    the bounds are achievable before the device is held to them."""
    kernel = nc.closed_kernel(a)
    X, Z = nc.grid(n), nc.rhs(n)
    K = nc.sk_matrix(kernel, X)
    s = nc.closed_scale(a)
    np.testing.assert_array_equal(K, s * np.eye(n))
    np.testing.assert_array_equal(cpu.kernel_matrix(_desc(kernel), X, diag_add=nc.NUGGET), K)
    cf = nc.closed_form(Z, a)
    G, sld, info = cpu.lml_batch([_desc(kernel)], X, Z, nc.NUGGET)
    assert info[0] == 0
    ratios = nc.closed_ratios(cf, G[0], sld[0])
    assert all(r <= 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("a", (nc.CLOSED_A, 0.0))
@pytest.mark.parametrize("n", nc.GRADIENT)
def test_closed_form_gradient_reference_inside_the_bounds(cpu, n, a):
    kernel = nc.closed_kernel(a)
    order = nc.gradient_order(kernel)
    assert order == (["amplitude", "length", "white"] if a else ["length", "white"])
    X, Z = nc.grid(n), nc.rhs(n)
    cf = nc.closed_form(Z, a)
    G, sld, info, trace, H = cpu.lml_grad(_desc(kernel), describe_gradient(kernel, 1), X, Z, nc.NUGGET)
    assert info == 0
    p = order.index("length")
    assert trace[p] == 0.0 and not np.any(H[p])
    ratios = nc.closed_ratios(cf, G, sld, trace, H, order)
    assert all(r <= 1.0 for r in ratios.values()), ratios


# ---- uplo = 'L' ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (129, 257))
def test_upper_triangle_never_read_cpu(cpu, n):
    A = nc.sk_matrix(nc.dense(), nc.grid(n))
    Z = nc.rhs(n)
    M = cpu.upload(A)
    assert cpu.potrf(M) == 0
    L0, (G0, sld0) = M.to_host(), cpu.forward_gram(M, Z)
    for r, c in nc.upper_plants(n):
        B = A.copy()
        B[r, c] = np.nan
        assert nc.dpotf2(B)[1] == 0
        M = cpu.upload(B)
        assert cpu.potrf(M) == 0
        np.testing.assert_array_equal(M.to_host(), L0)
        assert not np.any(np.triu(M.to_host(), 1))
        G, sld = cpu.forward_gram(M, Z)
        np.testing.assert_array_equal(G, G0)
        assert sld == sld0
