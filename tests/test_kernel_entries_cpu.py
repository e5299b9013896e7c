"""The entrywise truth of tests/kernel_entry_truth.py, validated without a device: the designs are exact, scikit-learn's float64 entries
are within REF_LIMIT eps of the long-double truth under the derived scale on EVERY case (so that e_dev <= BOUND max(e_ref, eps) on the
device is a bound of a few tens of eps per entry), the CPU backend's entries pass the device's bound, and three planted formula errors in
a float64 restatement do not.  The CPU backend takes its leaf values and derivatives from scikit-learn itself, so for a single leaf its
check repeats scikit-learn's; what it adds is the backend's own walk -- amplitude, constants, white noise, the sum, product and power
rules and the mapping of parameters onto K_gradient's columns.

Measured here (x86-64, numpy long double): e_ref <= 0.89 eps on every value and derivative entry of every case."""
import warnings

import numpy as np
import pytest

import gsum_amd
from gsum_amd._cpu import cpu_context
from gsum_amd._cpu import kernel_matrix as cpu_kernel_matrix

import kernel_entry_truth as kt

EPS = kt.EPS


@pytest.mark.parametrize("case", kt.ALL_CASES, ids=kt.CASE_IDS)
def test_design_is_exact_and_takes_the_path_it_names(case):
    kern, X, T, K, dK = kt.case_truth(case)
    kt.assert_exact_design(kern, X)
    desc, prm = gsum_amd.describe_kernel(kern, case.d), gsum_amd.kernels.describe_gradient(kern, case.d)
    assert (desc.n_ops > 0) == case.tree and len(prm) == len(T.d) == len(dK) <= 12


def test_every_order_and_every_leaf_class_is_in_the_matrix():
    for tree in (False, True):
        assert {c.n for c in kt.CASES if c.tree == tree} == set(kt.ONE_WORKGROUP) | set(kt.GENERAL)
    classes = {type(lf).__name__ + (str(getattr(lf, "nu", "")) if type(lf).__name__ == "Matern" else "")
               for c in kt.CASES if c.tree for lf in kt.leaf_kernels(c.kernel())}
    assert classes >= {"RBF", "Matern0.5", "Matern1.5", "Matern2.5", "Materninf", "RationalQuadratic", "ExpSineSquared", "DotProduct"}
    four = [c for c in kt.CASES if c.name == "four-aniso"]
    assert four and all(len(c.kernel().theta) == 12 for c in four)
    # every (leaf, dim) pair of the four anisotropic leaves has a length scale of its own in ITS dimension among the leaves ...
    ls = np.array([lf.length_scale for lf in kt.leaf_kernels(four[0].kernel())])
    assert ls.shape == (4, 2) and all(len(set(ls[:, m])) == 4 for m in range(2)) and all(a != b for a, b in ls)


@pytest.mark.parametrize("case", kt.ALL_CASES, ids=kt.CASE_IDS)
def test_scikit_learn_is_within_the_reference_limit_and_the_cpu_backend_within_the_bound(case):
    kern, X, T, K, dK = kt.case_truth(case)
    e_ref = [kt.entry_error(K, T.v, T.Sv)] + [kt.entry_error(dK[p], T.d[p], T.Sd[p]) for p in range(len(T.d))]
    print(f"{case.id}: e_ref / eps = " + " ".join(f"{e / EPS:.2f}" for e in e_ref))
    assert max(e_ref) <= kt.REF_LIMIT * EPS, (case.id, [e / EPS for e in e_ref])
    desc, prm = gsum_amd.describe_kernel(kern, case.d), gsum_amd.kernels.describe_gradient(kern, case.d)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        got = cpu_context().grad_entries(desc, prm, X)
        Kc = cpu_kernel_matrix(desc, X)
    assert kt.within_bound(kt.entry_error(Kc, T.v, T.Sv), e_ref[0])
    for p in range(len(prm)):
        assert kt.within_bound(kt.entry_error(got[p], T.d[p], T.Sd[p]), e_ref[1 + p]), (case.id, p)


def test_every_tree_kernel_has_its_two_argument_cases():
    assert {c.name for c in kt.TWO_ARG_CASES} == {name for name, _, _ in kt.TREES} and len(kt.TWO_ARG_CASES) == 2 * len(kt.TREES)
    for name, _, _ in kt.TREES:
        assert sorted(c.n <= 128 for c in kt.TWO_ARG_CASES if c.name == name) == [False, True]


@pytest.mark.parametrize("case", kt.TWO_ARG_CASES + [c for c in kt.CASES if not c.tree and c.n in (17, 129, 130)], ids=lambda c: c.id)
@pytest.mark.parametrize("m", kt.TWO_ARG_M)
def test_two_argument_truth_against_scikit_learn(case, m):
    kern, X, T, K, dK = kt.case_truth(case)
    Y = kt.lattice_points(m, case.d, seed=7) + 0.25
    v, Sv = kt.cross_truth(kern, X, Y)
    assert kt.entry_error(kern(X, Y), v, Sv) <= kt.REF_LIMIT * EPS


@pytest.mark.parametrize("case", kt.TWO_SCALE, ids=lambda c: c.id)
def test_two_scale_design_reaches_the_subnormal_band_and_beyond(case):
    kern, X, T, K, dK = kt.case_truth(case)
    far, band = kt.far_mask(case, X)
    assert far.sum() >= 1000 and band.sum() >= 100 and (~far & ~band).sum() >= 1000
    leafy = kt.leaf_parameters(T, far)
    assert leafy, "no parameter whose derivative vanishes with the leaf"
    for p in leafy:                                          # scikit-learn, the specification: exactly 0.0 out there, subnormal in the band
        assert np.all(dK[p][far] == 0.0) and np.all(np.isfinite(dK[p]))
    assert any(np.any((a[band] != 0.0) & (np.abs(a[band]) < kt.DBL_MIN)) for a in [K] + [dK[p] for p in leafy])


@pytest.mark.parametrize("exponent", [2, 0.5])
def test_cpu_backend_on_an_exponentiation_whose_base_underflows(exponent):
    """The CPU backend's walk of Exponentiation(RBF, e) + WhiteKernel where the base is exactly 0.0: its entries equal scikit-learn's
    under array_equal(equal_nan=True) -- NaN (0 * inf) in the length-scale column for e = 0.5, and the white-noise column, which the
    Exponentiation does not own, exactly zero there (e K^(e-1) = inf scales the Exponentiation's own parameters only)."""
    from sklearn.gaussian_process.kernels import RBF, Exponentiation, WhiteKernel
    kern = Exponentiation(RBF(0.25), exponent) + WhiteKernel(0.5)
    X = kt.two_scale_points(128)
    desc, prm = gsum_amd.describe_kernel(kern, 1), gsum_amd.kernels.describe_gradient(kern, 1)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        K, dK = kern(X, eval_gradient=True)
        got = cpu_context().grad_entries(desc, prm, X)
    assert np.count_nonzero(RBF(0.25)(X) == 0.0) > 1000 and (exponent != 0.5 or np.isnan(dK[:, :, 0]).any())
    assert not np.isnan(dK[:, :, 1]).any()
    for p in range(2):
        assert np.array_equal(got[p], dK[:, :, p], equal_nan=True), p


# ---- three planted errors in a float64 restatement of scikit-learn's formulas -------------------------------------------------------
def _restated(kind, X, plant=False):
    """float64, operation for operation like kernels.py; ``plant``: the formula error of that kind."""
    X = np.asarray(X, dtype=float)
    if kind == "rq":                                         # RationalQuadratic(0.5, 0.75): d / d log length_scale;  planted: 1 / base dropped
        ls, alpha = 0.5, 0.75
        q = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
        base = 1 + q / (2 * alpha * ls ** 2)
        K = base ** -alpha
        np.fill_diagonal(K, 1)
        return q * K / (ls ** 2) if plant else q * K / (ls ** 2 * base)
    if kind == "m52":                                        # Matern(0.5, nu=2.5);  planted: 5 / 3 -> 1.6666
        D = ((X[:, None, :] - X[None, :, :]) / 0.5) ** 2
        tmp = np.sqrt(5 * D.sum(-1))
        return ((1.6666 if plant else 5.0 / 3.0) * D * (tmp + 1)[..., None] * np.exp(-tmp)[..., None])[:, :, 0]
    ls = np.array([0.5, 2.0])                                # RBF([0.5, 2.0]): d / d log length_scale[0];  planted: the other dimension's D
    D = ((X[:, None, :] - X[None, :, :]) / ls) ** 2
    K = np.exp(-0.5 * D.sum(-1))
    np.fill_diagonal(K, 1)
    return K * D[:, :, 1 if plant else 0]


@pytest.mark.parametrize("kind,expr,d,p", [("rq", "RQ(length_scale=0.5, alpha=0.75)", 1, 1), ("m52", "Matern(0.5, nu=2.5)", 1, 0),
                                           ("swap", "RBF([0.5, 2.0])", 2, 0)])
def test_planted_errors_exceed_the_bound(kind, expr, d, p):
    case = kt.Case("planted-" + kind, 17, d, expr, kind == "rq")
    kern, X, T, K, dK = kt.case_truth(case)
    e_ref = kt.entry_error(dK[p], T.d[p], T.Sd[p])
    assert e_ref <= kt.REF_LIMIT * EPS
    good = kt.entry_error(_restated(kind, X), T.d[p], T.Sd[p])
    bad = kt.entry_error(_restated(kind, X, plant=True), T.d[p], T.Sd[p])
    print(f"{kind}: e_ref {e_ref / EPS:.2f} eps, restated {good / EPS:.2f} eps, planted {bad / EPS:.3g} eps")
    assert kt.within_bound(good, e_ref)
    assert not kt.within_bound(bad, e_ref) and bad > 1e6 * kt.BOUND * EPS
