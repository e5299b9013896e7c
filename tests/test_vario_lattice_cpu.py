"""The lattice designs of tests/vario_lattice.py without a GPU: the committed truth (tests/golden/vario_lattice_truth.json) against
a fresh mpmath evaluation, and backend='cpu' against the closed forms of the pair stage and against the truth of the cov sums.

CPU_TRUTH_RTOL is a measurement, not a derivation: SciPy's hyp2f1 in _cpu_cov_sum is what separates backend='cpu' from the truth.
The worst |cpu - truth| / E over all cases measured 3.1e-13 (scipy 1.15.3, the N = 120 case); the bound is ten times that."""
import warnings

import numpy as np
import pytest

import gsum_amd as gm
import vario_lattice as vl
from conftest import load_golden

CPU_TRUTH_RTOL = 3.1e-12


@pytest.fixture(scope="module")
def golden():
    return load_golden("vario_lattice_truth.json")["cases"]


def test_constants_are_the_class_constants():
    assert vl.VAR_FACTOR == gm.VariogramFourthRoot.var_factor and vl.CORR_FACTOR == gm.VariogramFourthRoot.corr_factor


def test_fixture_matches_a_fresh_truth(golden):
    pytest.importorskip("mpmath")
    fresh = vl.make_fixture()["cases"]
    assert sorted(fresh) == sorted(golden)
    for name, want in fresh.items():
        got = golden[name]
        for key in ("N", "nc", "variant", "requests", "M", "gt_sha256"):
            assert got[key] == want[key], (name, key)
        assert ("gt" in got) == ("gt" in want)
        for key in ("sum", "E", "sq", "sens") + (("gt",) if "gt" in want else ()):
            np.testing.assert_allclose(vl.A(got[key]), vl.A(want[key]), rtol=1e-25, atol=0, err_msg=f"{name} {key}")


def test_model_bits_and_case_shapes(golden):
    for name, (N, nc, variant, requests) in vl.CASES.items():
        rec = golden[name]
        gt = vl.model_gt(N, nc, variant)
        assert gt.min() > 0 and vl.gt_digest(gt) == rec["gt_sha256"]
        if "gt" in rec:
            np.testing.assert_array_equal(gt, vl.A(rec["gt"]))
        assert [tuple(r) for r in rec["requests"]] == requests and all(a <= b for a, b in requests)
    np.testing.assert_array_equal(vl.model_gt(600, 5), vl.A(golden["groups"]["gt"])[:, :5])
    assert [600 - k for k in vl.EDGE_BINS] == [513, 512, 511, 257, 256, 255, 2, 1]
    P = 600 * 599 // 2
    assert P == 179700 and -(-P // 4096) == 44


def test_cpu_pair_stage_on_the_lattice():
    N = 600
    X, bounds = vl.lattice(N)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        v = gm.VariogramFourthRoot(X, np.eye(N), bounds, backend="cpu")
    m = vl.counts_exact(N)
    np.testing.assert_array_equal(v.bin_counts, m)
    np.testing.assert_array_equal(v.bin_locations[1:], np.arange(1., N))
    mean = vl.indicator_dij_exact(N, np.arange(N))[1:] / m[1:, None]
    assert np.all(np.abs(v.gamma_star_hat[1:] - mean) <= np.spacing(mean))
    assert np.all(np.isnan(v.gamma_star_hat[0]))


@pytest.mark.parametrize("name", list(vl.CASES))
def test_cpu_cov_sums_against_the_truth(golden, name):
    N, nc, variant, requests = vl.CASES[name]
    t = vl.Truth(golden[name])
    X, bounds = vl.lattice(N)
    v = gm.VariogramFourthRoot(X, np.eye(N)[:nc], bounds, backend="cpu")
    np.testing.assert_array_equal(v.bin_counts, vl.counts_exact(N))
    v.gamma_tilde = vl.model_gt(N, nc, variant)
    worst = 0.
    for k1, k2 in requests:
        want = t.row(k1, k2)
        for a, b in ((k1, k2), (k2, k1)):
            got = v._cpu_cov_sum(a, b)
            worst = max(worst, float(np.max(np.abs(got - want.sum) / want.E)))
    print(f"{name}: worst |cpu - truth| / E = {worst:.2e}")
    assert worst <= CPU_TRUTH_RTOL
