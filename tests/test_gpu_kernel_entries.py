"""Every entry of the kernel matrix and of its derivative matrices dR_p = d kernel(X) / d log theta_p, as the PRODUCTION kernels computed
them, against long-double truth (run with ``-m gpu`` on an MI355X).  The derivative entries are read back from where ``gsum_lml_grad``
left them (``HipContext.grad_entries``: gsum_debug_grad_entries of the lab build): the n x n square of k_grad_small<TREE> for n <= 128,
the stored lower triangle of k_grad_contract<TREE, R, true> from n = 129 (and below it with option small_path = 0) -- every route that
calls gs_kernel_grad, gs_leaf_dlog_ls, gs_leaf_eval and gs_tree_eval.  The value entries come from ``kernel_matrix`` (k_build2 /
k_build_tree, one- and two-argument form).

Designs, truth, the error scale S of an entry and the case matrix: tests/kernel_entry_truth.py (validated without a device by
tests/test_kernel_entries_cpu.py, where scikit-learn's entries are within 0.89 eps of the truth on every case).  Per case, parameter and
route:  e = max over entries |x - truth| / S,  e_dev <= 16 max(e_ref, eps).  Structural properties are exact: S is zero on the diagonal of
a leaf derivative and off the diagonal of the white-noise derivative, so those entries must be 0.0; constant and white-noise derivatives
equal their weights; the one-workgroup square is symmetric; the general path's triangle equals the one-workgroup square bit for bit.
Every e_dev / eps and e_ref / eps goes to the parity record; the worst per route are in DESIGN.md section 9.1."""
import ctypes
import warnings

import numpy as np
import pytest

from conftest import record_parity

pytestmark = pytest.mark.gpu

import gsum_amd  # noqa: E402

import kernel_entry_truth as kt  # noqa: E402

EPS = kt.EPS
NUGGET = 1.0            # R = kernel(X) + I is positive definite whatever the kernel; the entries of dR_p do not depend on it


@pytest.fixture(scope="module")
def lab():
    return gsum_amd.lab_context(0)


def describe(kern, d):
    return gsum_amd.describe_kernel(kern, d), gsum_amd.kernels.describe_gradient(kern, d)


_DEVICE = {}


def device_entries(lab, case, route):
    """(P, n, n) derivative entries of a case on a route: "default" (one workgroup up to n = 128, the general path above) or "general"
    (small_path = 0).  One read-out per case, route and session."""
    key = (case.id, route)
    if key not in _DEVICE:
        kern, X, T, K, dK = kt.case_truth(case)
        desc, prm = describe(kern, case.d)
        assert (desc.n_ops > 0) == case.tree and len(prm) == len(T.d)
        rhs = np.ones((case.n, 1))
        try:
            lab.set_option("small_path", 0 if route == "general" else 1)
            _DEVICE[key] = lab.grad_entries(desc, prm, X, rhs, NUGGET)
        finally:
            lab.set_option("small_path", 1)
        _DEVICE[key].setflags(write=False)
    return _DEVICE[key]


def _is_structural(d):
    """A derivative that is a constant matrix or a multiple of the identity (additive constant, white noise): the device must return it
    exactly."""
    dg = np.diag(d)
    return bool(np.ptp(d) == 0 or (np.ptp(dg) == 0 and np.count_nonzero(d - np.diag(dg)) == 0))


def judge(case, route, got):
    kern, X, T, K, dK = kt.case_truth(case)
    over = []
    for p in range(len(T.d)):
        e_dev = kt.entry_error(got[p], T.d[p], T.Sd[p])
        e_ref = kt.entry_error(dK[p], T.d[p], T.Sd[p])
        record_parity(f"kernel_entries/{route}/{case.id}/p{p}", e_dev_eps=e_dev / EPS, e_ref_eps=e_ref / EPS)
        assert e_ref <= kt.REF_LIMIT * EPS
        if not kt.within_bound(e_dev, e_ref):
            over.append(f"{case.id}/{route}/p{p}: e_dev {e_dev / EPS:.3g} eps, e_ref {e_ref / EPS:.3g} eps")
        if _is_structural(T.d[p]):
            assert np.array_equal(got[p], T.d[p].astype(np.float64)), (case.id, route, p)
        exact0 = np.asarray(T.Sd[p] == 0)                # the diagonal of a leaf derivative, white noise off the diagonal, n = 1
        assert np.all(got[p][exact0] == 0.0), (case.id, route, p)
        assert exact0[np.diag_indices(case.n)].all() or np.all(np.diag(T.d[p]) != 0), (case.id, p)
    return over


@pytest.mark.parametrize("case", kt.ALL_CASES, ids=kt.CASE_IDS)
def test_gradient_entries_against_truth(lab, case):
    """Default options: k_grad_small<false | true> at n = 1, 2, 15, 16, 17, 127, 128, k_grad_contract<false, 2, true> | <true, 1, true> at
    129, 130, 191, 193, 257 -- the flattened family at d = 1, 2, 3, 8 (every length scale different), every leaf class alone and under
    C *, RationalQuadratic at alpha = 0.75 and 48, ExpSineSquared(1, 3) and (0.5, 0.75), Matern(inf), C * DotProduct, Exponentiation 2
    and 3, a product, a sum of products, four anisotropic leaves with amplitudes (12 parameters), and the two-scale designs."""
    got = device_entries(lab, case, "default")
    over = judge(case, "default", got)
    if case.n <= 128:
        for p in range(len(got)):
            assert np.array_equal(got[p], got[p].T), (case.id, p)            # the one-workgroup square: lower == upper
    assert not over, "\n".join(over)


@pytest.mark.parametrize("case", [c for c in kt.ALL_CASES if c.n <= 128], ids=lambda c: c.id)
def test_general_path_triangle_equals_the_one_workgroup_square(lab, case):
    """The orders both routes can run (small_path = 0): the general path against the truth too, and bit for bit against k_grad_small."""
    small = device_entries(lab, case, "default")
    general = device_entries(lab, case, "general")
    over = judge(case, "general", general)
    assert np.array_equal(np.tril(general), np.tril(small), equal_nan=True), case.id
    assert not over, "\n".join(over)


@pytest.mark.parametrize("case", kt.TWO_SCALE, ids=lambda c: c.id)
def test_far_entries_are_exactly_zero(lab, case):
    """A fine cluster plus points tens of length scales away: where the exp argument is beyond -745.2 every derivative that carries the
    leaf's exponential is exactly 0.0, nothing is NaN, and the subnormal band in between is under the bound (test above)."""
    kern, X, T, K, dK = kt.case_truth(case)
    far, band = kt.far_mask(case, X)
    got = device_entries(lab, case, "default")
    assert np.all(np.isfinite(got))
    leafy = kt.leaf_parameters(T, far)
    assert leafy
    for p in leafy:
        assert np.all(got[p][far] == 0.0), (case.id, p, np.abs(got[p][far]).max())


def _value_check(label, kern, got, ref, v, Sv, claimed=None):
    """``claimed``: the entries the header's claim covers (None: all; the two-scale designs: kernel_entry_truth.table_range)."""
    e_dev, e_ref = kt.entry_error(got, v, Sv), kt.entry_error(ref, v, Sv)
    claim = kt.value_claim(kern)
    claimed = np.ones(got.shape, bool) if claimed is None else claimed
    ulps = kt.ulps_apart(got[claimed], ref[claimed])
    record_parity(f"kernel_entries/value/{label}", e_dev_eps=e_dev / EPS, e_ref_eps=e_ref / EPS, ulps_from_sklearn=ulps,
                  ulps_from_sklearn_anywhere=kt.ulps_apart(got, ref), claim=str(claim))
    assert e_ref <= kt.REF_LIMIT * EPS
    assert kt.within_bound(e_dev, e_ref), f"{label}: e_dev {e_dev / EPS:.3g} eps, e_ref {e_ref / EPS:.3g} eps"
    if claim == "bits":
        assert np.array_equal(got[claimed], ref[claimed]), f"{label}: {ulps} ulps from scikit-learn's matrix"
    elif claim == "ulps2":
        assert ulps <= 2, f"{label}: {ulps} ulps from scikit-learn's matrix"


@pytest.mark.parametrize("case", kt.ALL_CASES, ids=kt.CASE_IDS)
def test_value_entries_one_argument(lab, case):
    """kernel_matrix(desc, X): the truth's bound, array_equal to scikit-learn where the header of build.hip.h claims bit identity (on the
    two-scale designs: outside the band of subnormal exponentials, which the header leaves to the device library's exp), <= 2 ulps for a
    RationalQuadratic leaf."""
    kern, X, T, K, dK = kt.case_truth(case)
    desc, _ = describe(kern, case.d)
    claimed = kt.table_range(case, X) if case.design == "two_scale" else None
    _value_check(f"{case.id}/one", kern, lab.kernel_matrix(desc, X), K, T.v, T.Sv, claimed)


@pytest.mark.parametrize("m", kt.TWO_ARG_M)
@pytest.mark.parametrize("case", kt.TWO_ARG_CASES, ids=lambda c: c.id)
def test_value_entries_two_arguments(lab, case, m):
    """kernel_matrix(desc, X, Y) of EVERY tree kernel of the matrix, at one one-workgroup order and one general-path order each, with
    m = 1, 127 and 129 columns (k_build_tree<true>: one column, one short of a 128-column tile, one past it), Y on the lattice, shifted by
    a quarter."""
    kern, X, T, K, dK = kt.case_truth(case)
    desc, _ = describe(kern, case.d)
    Y = kt.lattice_points(m, case.d, seed=7) + 0.25
    v, Sv = kt.cross_truth(kern, X, Y)
    _value_check(f"{case.id}/m{m}", kern, lab.kernel_matrix(desc, X, Y), kern(X, Y), v, Sv)


@pytest.mark.parametrize("n", [128, 193])
@pytest.mark.parametrize("exponent", [2, 0.5])
def test_exponentiation_of_a_base_that_underflows_to_zero(lab, n, exponent):
    """K ** e where the base is exactly 0.0 out there: e = 2 gives 0 with derivative 0; e = 0.5 gives 0 with derivative 0 * inf = NaN in
    scikit-learn, which is the specification (describe_gradient: parameter p IS K_gradient[:, :, p]).  On every entry whose base
    underflowed the device's value and derivatives equal scikit-learn's under array_equal(equal_nan=True) -- the same zeros, the same
    NaNs; the white-noise column, which the Exponentiation does not own, is exactly zero there (an Exponentiation scales the derivatives
    of its own parameters only: e K^(e-1) = inf must not reach the others' zeros).  The other entries are under the truth's bound; against
    scikit-learn they are NOT bit-identical in general (numpy squares and takes square roots for the exponents 2 and 0.5, the device
    calls pow(): measured, one ulp on 11-20 % of the value entries, at most two on 6-10 % of the length-scale derivative's, with the same
    e_dev as e_ref to two digits), and how far apart they are goes to the parity record."""
    from sklearn.gaussian_process.kernels import RBF, Exponentiation, WhiteKernel
    kern = Exponentiation(RBF(0.25), exponent) + WhiteKernel(0.5)
    X = kt.two_scale_points(n)
    kt.assert_exact_design(kern, X)
    desc, prm = describe(kern, 1)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        K, dK = kern(X, eval_gradient=True)
        under = RBF(0.25)(X) == 0.0
    assert under.sum() > 1000 and (exponent != 0.5 or np.isnan(dK[:, :, 0][under]).all())
    got = lab.grad_entries(desc, prm, X, np.ones((n, 1)), NUGGET)
    Kd = lab.kernel_matrix(desc, X)
    T = kt.entries_truth(kern, X)
    assert np.array_equal(Kd[under], K[under])
    rest = ~under
    e_dev, e_ref = kt.entry_error(Kd[rest], T.v[rest], T.Sv[rest]), kt.entry_error(K[rest], T.v[rest], T.Sv[rest])
    figures = dict(value_e_dev_eps=e_dev / EPS, value_e_ref_eps=e_ref / EPS, value_entries_not_bit_identical=int(np.sum(Kd[rest] != K[rest])),
                   value_ulps_from_sklearn=kt.ulps_apart(Kd[rest], K[rest]))
    ok = e_ref <= kt.REF_LIMIT * EPS and kt.within_bound(e_dev, e_ref)
    for p in range(len(prm)):
        assert np.array_equal(got[p][under], dK[:, :, p][under], equal_nan=True), (n, exponent, p)
        e_dev = kt.entry_error(got[p][rest], T.d[p][rest], T.Sd[p][rest])
        e_ref = kt.entry_error(dK[:, :, p][rest], T.d[p][rest], T.Sd[p][rest])
        figures.update({f"p{p}_e_dev_eps": e_dev / EPS, f"p{p}_e_ref_eps": e_ref / EPS,
                        f"p{p}_entries_not_bit_identical": int(np.sum(got[p][rest] != dK[:, :, p][rest])),
                        f"p{p}_ulps_from_sklearn": kt.ulps_apart(got[p][rest], dK[:, :, p][rest])})
        ok = ok and e_ref <= kt.REF_LIMIT * EPS and kt.within_bound(e_dev, e_ref)
    record_parity(f"kernel_entries/pow_underflow/n{n}-e{exponent}", entries_underflowed=int(under.sum()), **figures)
    assert ok, figures


def test_the_read_out_refuses_what_it_cannot_vouch_for(lab):
    """gsum_debug_grad_entries never reads stale memory: it refuses after release_scratch, after a batch call, with grad_split = 0, for
    another order, and -- on the one-workgroup path -- for any parameter but the last."""
    case = next(c for c in kt.CASES if c.name == "rbf-amp-w-add" and c.n == 130)
    small = next(c for c in kt.CASES if c.name == "rbf-amp-w-add" and c.n == 17)
    def read(p, n):
        out = np.full((n, n), np.nan)
        rc = lab._lib.gsum_debug_grad_entries(lab._h, p, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n)
        return rc, out

    for c in (case, small):
        kern, X, T, K, dK = kt.case_truth(c)
        desc, prm = describe(kern, c.d)
        rhs = np.ones((c.n, 1))
        last = len(prm) - 1
        want = device_entries(lab, c, "default")[last]
        assert lab.lml_grad(desc, prm, X, rhs, NUGGET)[2] == 0
        rc, out = read(last, c.n)
        assert rc == 0 and np.array_equal(np.tril(out), np.tril(want))
        if c.n > 128:
            assert np.all(np.triu(out, 1) == 0.0)                                   # the stored triangle: nothing above the diagonal
            rc0, first = read(0, c.n)                                               # ... and every parameter can be read
            assert rc0 == 0 and np.all(np.triu(first, 1) == 0.0)
            assert np.array_equal(np.tril(first), np.tril(device_entries(lab, c, "default")[0]))
        else:
            assert read(0, c.n)[0] == -2                                            # the last parameter only
        assert read(last, c.n + 1)[0] == -2 and read(len(prm), c.n)[0] == -2 and read(-1, c.n)[0] == -2
        lab.set_option("release_scratch", 1)
        assert read(last, c.n)[0] == -2
        assert lab.lml_grad_batch([desc], [prm], X, rhs, NUGGET)[2][0] == 0          # a batch call, even of one
        assert read(last, c.n)[0] == -2
        lab.lml_grad(desc, prm, X, rhs, NUGGET)
        assert read(last, c.n)[0] == 0
        lab.kernel_matrix(desc, X)                                                  # another call has reserved a work buffer since
        assert read(last, c.n)[0] == -2
    kern, X, T, K, dK = kt.case_truth(case)
    desc, prm = describe(kern, case.d)
    try:
        lab.set_option("grad_split", 0)
        lab.lml_grad(desc, prm, X, np.ones((case.n, 1)), NUGGET)
        with pytest.raises(ValueError, match="grad_split"):
            lab._check(read(0, case.n)[0])
    finally:
        lab.set_option("grad_split", 1)
