"""libgsum_toep.so on the device: the shared cases of toeplitz_cases.py on backend='hip', the first column against the dense device build,
the reference's notebook grid and S2 / S3 known answers through ``structure="toeplitz"``.  Achieved distances go to the parity record."""
import numpy as np
import pytest
from scipy.linalg import toeplitz
from sklearn.gaussian_process.kernels import RBF, Matern, WhiteKernel

from conftest import load_golden, record_parity

import gsum_amd as gm  # noqa: E402
import toeplitz_cases as tc  # noqa: E402
from toeplitz_cases import notebook_process  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", tc.SIZES)
def test_closed_form_sizes(n):
    got, cpu = tc.check_closed_form("hip", n)
    record_parity(f"toeplitz/closed_form/n{n}", G_eps=got[0] / tc.EPS, sld_eps=got[1] / tc.EPS, cpu_G_eps=cpu[0] / tc.EPS, cpu_sld_eps=cpu[1] / tc.EPS)


@pytest.mark.parametrize("n,c,n_sets,m", tc.SHAPES)
def test_closed_form_shapes(n, c, n_sets, m):
    tc.check_closed_form("hip", n, c, n_sets, m)


def test_the_limit_is_reported_and_enforced():
    from gsum_amd import toeplitz
    n = toeplitz.toeplitz_max_n("hip")
    assert n == tc.SIZES[-1] == 8192                                    # the largest size of the closed-form cases is the limit
    with pytest.raises(ValueError, match="n must be <= 8192"):
        gm.toeplitz_gram(tc.kms_column(n + 1, 0.5), np.ones((n + 1, 1)))


def test_n8192_seven_columns_against_the_closed_form():
    got, cpu = tc.check_closed_form("hip", 8192, 7, 1, 1)
    record_parity("toeplitz/closed_form/n8192_c7", G_eps=got[0] / tc.EPS, sld_eps=got[1] / tc.EPS)


def test_failures():
    tc.check_failures("hip")


def test_properties():
    tc.check_properties("hip")


@pytest.mark.parametrize("name", tc.ill_names())
def test_ill_conditioned_goldens(name):
    """Distance from the mpmath truth: at most numpy's dense Cholesky's on the same T, and within 4 x the cpu backend's (floor 64 * 2^-53).
    Measured on an MI355X, G relative to max|G| (device / numpy / cpu): rbf_n64 6.4e-13 / 1.1e-6 / 8.6e-10, rbf_n128 7.5e-13 / 1.4e-6 /
    3.5e-9, matern52_n64 3.1e-15 / 2.5e-11 / 2.5e-15, matern52_n128 2.4e-14 / 2.5e-9 / 2.5e-13, rbf_white_n128 3.5e-14 / 2.2e-8 / 2.0e-11;
    sum_log_diag 0 to 2e-16.  matern52_n64 is the case that needs the correction word for the low words of L:
    without it the device sits at 4.2e-14, above 4 x max(cpu, floor) = 2.8e-14.
    The goldens of toeplitz_classes.json (the smallest n of the classes with 4, 8 and 16 elements per thread, the last with v in LDS
    and two column chunks; truth by the mpmath Schur recursion): matern52_n513 (cond 1.4e12) 3.6e-14 / 9.1e-7 / 4.9e-9, rbf_n2049
    (nugget 1e-8, cond 9.0e10) 1.1e-13 / 3.4e-8 / 3.7e-10, matern52_n4097 (cond 1.7e13) 1.5e-13 / 3.7e-6 / 1.2e-8; sum_log_diag 0."""
    d, d_np, d_cpu = tc.check_ill("hip", name)
    record_parity(f"toeplitz/golden/{name}", G=d[0], sld=d[1], numpy_G=d_np[0], numpy_sld=d_np[1], cpu_G=d_cpu[0], cpu_sld=d_cpu[1])


@pytest.mark.parametrize("n", [n for n in tc.SIZES if n >= 3])
def test_arfima_sizes(n):
    """ARFIMA(0, d, 0), d over (0.4, -0.3): reflection coefficients d / (k - d), so every step rotates and v, its LDS home in the
    largest class and the publication of v[k+2] carry numbers instead of zeros.  sum_log_diag against the closed form at every size.
    G against an mpmath golden at n = 513, 2049, 4097 and 8192 (all four were generated); at the other sizes against the cpu backend's
    G within the sum of the two bounds, 2 * 4 * 64 * 2^-53 of max|G|, which is a comparison of two implementations and not a truth."""
    record_parity(f"toeplitz/arfima/n{n}", **tc.check_arfima("hip", n))


@pytest.mark.parametrize("n", tc.LATE_SIZES)
def test_late_failures(n):
    """The first failing step placed at the first steps, around a thread boundary (E, J E), and in the last two steps of the classes
    with E = 4, 8 and 16 generator elements per thread."""
    info = tc.check_late_failures("hip", n)
    record_parity(f"toeplitz/late_failures/n{n}", info=info)


def test_first_columns_in_three_launches():
    info = tc.check_chunk_loop("hip")
    record_parity("toeplitz/chunk_loop", info=info, **tc.CHUNKED)


def test_scaling_is_bitwise():
    record_parity("toeplitz/scaling", sld_shift_eps=tc.check_scaling("hip") / tc.EPS)


@pytest.mark.parametrize("a", tc.FAR)
def test_far_scaling(a):
    """Right-hand sides scaled by 2^140 and 2^-140, outside what the fp32 correction word and the fp32 copy of y_k hold.  Before the
    columns were normalised on the device (k_colexp) the library returned non-finite G with info 0 at +140 and lost the correction at
    -140 (read from the code: (float)y overflows, ulf * yf underflows)."""
    d = tc.check_far_scaling("hip", a)
    record_parity(f"toeplitz/far_scaling/a{a}", G=d[0], sld=d[1])


def test_scale_of_t_outside_the_stated_range_is_refused():
    t = tc.kms_column(8, 0.5)
    for s in (2.0 ** -66, 2.0 ** 66):
        with pytest.raises(ValueError, match=r"t\[0\] must lie within"):
            gm.toeplitz_gram(s * t, np.ones((8, 1)))
    for s in (2.0 ** -64, 2.0 ** 64):
        assert gm.toeplitz_gram(s * t, np.ones((8, 1)))[2] == 0


@pytest.mark.parametrize("kernel", [RBF(0.2), Matern(0.3, nu=2.5), Matern(0.3, nu=0.5), 2.0 * RBF(0.2) + WhiteKernel(1e-3)], ids=str)
def test_toeplitz_column_is_the_dense_first_column(kernel):
    X = np.linspace(0, 1, 1031)[:, None]
    K = gm.default_context().kernel_matrix(gm.describe_kernel(kernel, 1), X)
    want = K[:, 0].copy()
    want[0] += 1e-10
    assert np.array_equal(gm.toeplitz_column(kernel, X, 1e-10), want)


def test_notebook_grid_known_answer(notebook_grid):
    """The reference's recorded 80 x 100 (Q, ell) scan through the structured path on the device: argmax (36, 39), rtol 1e-12."""
    g = notebook_grid
    gp, thetas = notebook_process(g, gm.TruncationGP, "hip")
    want = np.array(g["grid"])
    grids = [gp.log_marginal_likelihood_grid(thetas, g["ratio_vals"], mode=mode, structure="toeplitz") for mode in ("full", "reuse")]
    assert np.array_equal(grids[0], grids[1])
    grid = grids[0]
    assert list(np.unravel_index(np.argmax(grid), grid.shape)) == [36, 39]
    assert not np.isneginf(grid).any() and not np.isnan(grid).any()
    rel = float(np.max(np.abs(grid - want) / np.abs(want)))
    record_parity("toeplitz/notebook_grid_80x100", max_rel=rel)
    np.testing.assert_allclose(grid, want, rtol=1e-12)
    tp, _ = notebook_process(g, gm.TruncationTP, "hip")
    np.testing.assert_allclose(tp.log_marginal_likelihood_grid(thetas[::7], g["ratio_vals"][::9], structure="toeplitz"),
                               tp.log_marginal_likelihood_grid(thetas[::7], g["ratio_vals"][::9]), rtol=1e-12)


def _s_inputs(n, r, seed):
    X = 0.1 * np.arange(n)[:, None]
    c = np.random.RandomState(seed).randn(n, r)
    return X, gm.partials(c, ratio=0.5, ref=1.0, orders=np.arange(r))


@pytest.mark.parametrize("n", [512, 2048])
def test_large_known_answers(large_lml, n):
    """S2 / S3 (0.1 * arange(n), RBF(0.2), nugget 1e-10, lambda_min about 2.7e-8).  The structured path answers for the exactly Toeplitz
    matrix T of the first column, the reference for kernel(X), whose diagonals differ in their last bits: conditioning times that
    defect.  So against the reference's value the bound is 4 x the distance of numpy's dense Cholesky applied to T (numpy alone; about
    7e-10), and against the extended-precision value of T itself (tests/golden/toeplitz.json) it is 1e-10."""
    case = [c for c in large_lml if c["n"] == n][0]
    r = case["r"]
    X, y = _s_inputs(n, r, case["seed"])
    orders = np.arange(r)
    gp = gm.TruncationGP(kernel=RBF(case["length_scale"]), ratio=0.5, ref=1.0, center=0, disp=0, df=1, scale=1, optimizer=None)
    gp.X_train_, gp.y_train_, gp.orders_ = X, y, orders
    theta = np.log([case["length_scale"]])
    qs = [float(q) for q in case["lml"]]
    got = gp.log_marginal_likelihood_grid([theta], qs, structure="toeplitz")[:, 0]
    # the yardstick: numpy's Cholesky of the Toeplitz matrix of the same first column, the same host algebra
    t = gm.toeplitz_column(RBF(case["length_scale"]), X, gp.coeffs_process.nugget)
    L = np.linalg.cholesky(toeplitz(t))
    sld = float(np.sum(np.log(np.diag(L))))
    truth = {c["ratio"]: c for c in tc.golden()["large"] if c["n"] == n}
    t_gold = tc.hex_column([c for c in truth.values() if "t_hex" in c][0])
    from scipy.linalg import solve_triangular
    for (qk, want), mine in zip(case["lml"].items(), got):
        q = float(qk)
        coeffs, det = gp._coeffs_and_jacobian(X, y, orders, {"ratio": q})
        Z = np.concatenate([coeffs, np.ones((n, 1))], axis=1)
        W = solve_triangular(L, Z, lower=True)
        yard = gm.lml_from_gram(W.T @ W, sld, n, 0, 0, 1, 1)[0] - det
        d_yard, d_mine = abs(yard - want) / abs(want), abs(mine - want) / abs(want)
        # the extended-precision value of T: the golden's own first column through the library and the same host algebra
        G, s, info = gm.toeplitz_gram(t_gold, Z)
        assert info == 0
        d_truth = abs(gm.lml_from_gram(G[0], s, n, 0, 0, 1, 1)[0] - det - truth[q]["lml_truth_f64"]) / abs(truth[q]["lml_truth_f64"])
        record_parity(f"toeplitz/large/n{n}_q{q}", vs_reference=d_mine, numpy_on_T_vs_reference=d_yard, vs_truth_on_T=d_truth,
                      column_equals_golden=bool(np.array_equal(t, t_gold)))
        assert d_mine <= 4 * d_yard, (n, q, d_mine, d_yard)
        assert d_truth <= 1e-10, (n, q, d_truth)
