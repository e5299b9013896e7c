"""libgsum_band.so on the device: the band against the dense device build, the exact factors, the derived bounds, failures, independence
of the batch and of the stored width, and ``structure="banded"`` against the long-double truth and the dense route (banded_cases.py;
DESIGN.md section 26).  Every edge comes from gsum_band_block() and gsum_band_max_halfwidth().  Achieved figures go to the parity record."""
import numpy as np
import pytest
from sklearn.gaussian_process.kernels import RBF, Matern

from conftest import have_gpu, record_parity

import banded_cases as bc  # noqa: E402
import gsum_amd as gm  # noqa: E402
from gsum_amd import _band_lib  # noqa: E402

pytestmark = pytest.mark.gpu

# The cases are parametrised by the library's constants, so the library is loaded while the suite is collected.  PyTorch goes first,
# as it does for every other module (conftest asks it for the device before a test runs): the HIP runtime PyTorch brings must be the
# process's one, or the libraries loaded later find no device.
have_gpu()
B, W = _band_lib.block(), _band_lib.max_halfwidth()


# ---- 1. build ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ("flat", "tree"))
@pytest.mark.parametrize("points", ("uniform", "clustered"))
def test_band_equals_the_dense_device_build(kernel, points):
    k = bc.bench_kernel() if kernel == "flat" else bc.tree_kernel()
    X = (bc.uniform_points(300) if points == "uniform" else bc.clustered_points(300))[:, None]
    desc = gm.describe_kernel(k, 1)
    K = gm.default_context().kernel_matrix(desc, X, X)
    b = gm.banded_halfwidth(k, X)
    assert b == bc.brute_halfwidth(K) and 0 < b <= W
    assert b == gm.banded_halfwidth(desc, X) == gm.banded_halfwidth(k, X, backend="cpu")
    AB = gm.banded_matrix(k, X, nugget=1e-6)
    assert AB.shape == (b + 1, 300)
    np.testing.assert_array_equal(AB[1:], bc.to_band(K, b)[1:])
    np.testing.assert_array_equal(AB[0], np.full(300, float(desc.one_arg_diagonal()) + 1e-6))
    i, j = np.indices(K.shape)
    assert not np.any(K[np.abs(i - j) > b]) and bc.rows_contiguous(K)
    wide = gm.banded_matrix(k, X, nugget=1e-6, halfwidth=b + 9)       # further diagonals: zeros, and zeros beyond the matrix
    np.testing.assert_array_equal(wide, bc.widen(AB, 9))


def test_the_widest_band_passes_and_one_more_is_refused():
    X = np.arange(W + 3.0)
    lo, hi = bc.length_scale_at_width(lambda ls: RBF(ls), X, W)
    assert gm.banded_halfwidth(RBF(lo), X) == W and gm.banded_matrix(RBF(lo), X).shape == (W + 1, W + 3)
    with pytest.raises(ValueError, match=f"half-bandwidth exceeds {W}"):
        gm.banded_halfwidth(RBF(hi), X)
    with pytest.raises(ValueError, match="half-bandwidth exceeds"):
        gm.banded_matrix(RBF(hi), X)
    with pytest.raises(ValueError, match="b must be between 0 and"):
        gm.banded_matrix(RBF(lo), X, halfwidth=W + 1)
    with pytest.raises(ValueError, match="b must be between 0 and"):
        gm.banded_gram(np.ones((W + 2, 8)), np.ones((8, 1)))


# ---- 2. exact factors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", bc.exact_widths(B, W))
def test_exact_factors(b):
    """(a): L, Y and G bit for bit the planted ones at every size around the block and the band, every column and set count."""
    worst = 0.0
    shapes = [(c, s) for c in (1, 5, 16) for s in (1, 3)]
    for k, n in enumerate(bc.exact_sizes(b, B)):
        for c, s in (shapes if n == bc.exact_sizes(b, B)[-1] else [shapes[k % 6], shapes[(k + 3) % 6]]):
            worst = max(worst, bc.check_exact("hip", n, b, c, s))
    record_parity(f"banded/exact/b{b}", sld_abs_err=worst)


# ---- 3. derived bounds ------------------------------------------------------------------------------------------------------------------
def test_derived_bounds_on_the_benchmark_band():
    AB = gm.banded_matrix(bc.bench_kernel(), bc.uniform_points(1025), nugget=bc.BENCH_NUGGET)
    assert AB.shape[0] == 78
    r = bc.check_bounds("hip", "bench n=1025", AB, bc.rough_curves(AB, 6), 1)
    record_parity("banded/bounds/bench_n1025", factor=r[0], substitution=r[1], gram=r[2])


def test_derived_bounds_at_the_widest_band():
    n = 2 * W + 3
    X = np.arange(float(n))
    lo, _ = bc.length_scale_at_width(lambda ls: Matern(ls, nu=2.5), X, W)
    AB = gm.banded_matrix(Matern(lo, nu=2.5), X, nugget=1e-8)
    assert AB.shape == (W + 1, n)
    r = bc.check_bounds("hip", f"matern52 b={W}", AB, bc.rough_curves(AB, 16), 2)
    record_parity("banded/bounds/matern52_widest", factor=r[0], substitution=r[1], gram=r[2])


def test_derived_bounds_on_clustered_points():
    AB = gm.banded_matrix(bc.tree_kernel(), bc.clustered_points(700))
    r = bc.check_bounds("hip", "tree clustered n=700", AB, bc.rough_curves(AB, 4), 1)
    record_parity("banded/bounds/tree_clustered", factor=r[0], substitution=r[1], gram=r[2])


# ---- 4. failures ------------------------------------------------------------------------------------------------------------------------
def test_failures():
    bc.check_failures("hip", B)


# ---- 5. independence --------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_batch_the_stored_width_or_the_chunk():
    n, b = 3 * B + 7, B + 5
    rng = np.random.default_rng(5)
    AB = 0.3 * rng.standard_normal((7, b + 1, n))                      # seven diagonally dominant bands
    AB[:, 0] = 2.0 + 0.6 * b + rng.random((7, n))
    Z = rng.standard_normal((n, 10))
    alone = gm.banded_gram(AB[3], Z, 2, return_factor=True)
    assert alone[2] == 0

    def same(got, i, wide=0):
        assert np.array_equal(got[0][i], alone[0]) and got[1][i] == alone[1] and got[2][i] == 0
        assert np.array_equal(got[3][i], bc.widen(alone[3], wide))

    same(gm.banded_gram(AB, Z, 2, return_factor=True), 3)
    same(gm.banded_gram(AB[::-1], Z, 2, return_factor=True), 3)
    same(gm.banded_gram(np.stack([bc.widen(a, 9) for a in AB]), Z, 2, return_factor=True), 3, wide=9)
    one = gm.banded_gram(bc.widen(AB[3], 9), Z, 2, return_factor=True)
    assert np.array_equal(one[0], alone[0]) and one[1] == alone[1] and np.array_equal(one[3], bc.widen(alone[3], 9))
    # two chunks of matrices, and the sets of a matrix in chunks
    h = _band_lib.default_handle(0)
    try:
        h.set_chunk(4 * (b + 1) * n)                                    # four matrices' bands; fewer than two matrices' solved columns
        same(gm.banded_gram(AB, Z, 2, return_factor=True), 3)
        h.set_chunk(n * 5)                                              # one matrix, one set at a time
        same(gm.banded_gram(AB, Z, 2, return_factor=True), 3)
        Y = gm.banded_forward(np.stack([alone[3]] * 3), Z)
        assert np.array_equal(Y[0], Y[2])
    finally:
        h.set_chunk(0)
    assert np.array_equal(gm.banded_forward(alone[3], Z), Y[0])
    assert set(h.times()) == set(_band_lib.PHASES) and h.times()["factor"] > 0


# ---- 6. the model layer -----------------------------------------------------------------------------------------------------------------
def test_model_value():
    d_truth, d_dense = bc.check_model("hip", 1025)
    record_parity("banded/model/n1025", truth_rel=d_truth, dense_rel=d_dense)


def test_a_matrix_that_does_not_factor_is_minus_infinity():
    X, y = bc.model_inputs(1025)
    gp = gm.ConjugateGaussianProcess(kernel=RBF(0.2), optimizer=None, nugget=-2.0)
    thetas = [np.log([0.2]), np.log([0.1])]
    assert np.all(gp.log_marginal_likelihood_batch(thetas, X=X[:200], y=y[:200], structure="banded") == -np.inf)
    tg = bc.truncation_process("hip", X[:200], y[:200])
    tg.coeffs_process.nugget = -2.0
    assert np.all(tg.log_marginal_likelihood_grid(thetas, [0.4, 0.5], structure="banded") == -np.inf)


def test_one_evaluation_beyond_the_dense_route():
    """n = 46 342, the first n whose square reaches 2^31 (the dense route takes no such matrix): the banded route against
    backend='cpu' at 1e-10."""
    n = 46342
    assert n * n >= 2 ** 31
    X = bc.uniform_points(n)[:, None]
    y = bc.rough_curves(gm.banded_matrix(bc.bench_kernel(), X, nugget=bc.BENCH_NUGGET, backend="cpu"), 3)[:, :2]      # drawn from the kernel itself
    th = np.log([0.2])
    got = bc.model_process("hip").log_marginal_likelihood(th, X=X, y=y, structure="banded")
    want = bc.model_process("cpu").log_marginal_likelihood(th, X=X, y=y, structure="banded")
    print(f"banded n={n}: hip {got!r}, cpu {want!r}, rel {bc.rel(got, want):.3g}")
    record_parity("banded/model/n46342", cpu_rel=bc.rel(got, want))
    assert bc.rel(got, want) <= 1e-10
