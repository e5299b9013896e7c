"""gsum_amd.Diagnostic / pivoted_cholesky on backend='cpu' against the reference's own outputs (tests/golden/diagnostics.json,
tests/golden/make_golden_diagnostics.py), their shapes and raising behaviour, and the C ABI entry point behind the device path."""
import base64
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import gsum_amd as gm
from gsum_amd import _lib


def _load():
    """tests/golden/diagnostics.json with its arrays decoded (float64 bytes, see make_golden_diagnostics.py) and every case's
    covariance rebuilt from its stored lower triangle"""
    def dec(v):
        if isinstance(v, dict) and "f64" in v:
            return np.frombuffer(base64.b64decode(v["f64"]), "<f8").reshape(v["shape"]).copy()
        if isinstance(v, dict):
            return {k: dec(x) for k, x in v.items()}
        if isinstance(v, list):
            return [dec(x) for x in v]
        return v
    data = dec(json.load(open(os.path.join(GOLDEN, "diagnostics.json"))))
    covs = {}
    for c in data["cases"]:
        if "cov_tril" in c:
            cov = np.zeros((c["n"], c["n"]))
            cov[np.tril_indices(c["n"])] = c["cov_tril"]
            covs[c["name"]] = cov + np.tril(cov, -1).T
        c["cov"] = covs[c.get("cov_of", c["name"])]
        c["cov0"] = 1.3 * c["cov"] + 0.01 * np.diag(np.diag(c["cov"]))     # make_golden_diagnostics.kl_cov0
    return data


DATA = _load()
CASES = DATA["cases"]


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def test_sqrt_errors_is_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "gsum_hip.h")).read()
    assert "int gsum_sqrt_errors(" in header
    assert "gsum_sqrt_errors" in _lib.PROTOTYPES
    assert hasattr(_lib.load_library(), "gsum_sqrt_errors")
    assert callable(getattr(_lib.HipContext, "sqrt_errors")) and callable(getattr(_lib.HipContext, "pstrf"))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cpu_diagnostic_matches_reference(case):
    mean, cov = np.array(case["mean"]), np.array(case["cov"])
    d = gm.Diagnostic(mean, cov, df=case["df"], random_state=1, backend="cpu")
    for tag in ("1", "3"):
        Y = np.array(case["Y" + tag])
        np.testing.assert_array_equal(d.individual_errors(Y), case["individual_errors_" + tag])
        np.testing.assert_array_equal(d.chi2(Y), case["chi2_" + tag])
        np.testing.assert_array_equal(d.credible_interval(Y, np.array(case["intervals"])), case["credible_interval_" + tag])
        assert rel(d.cholesky_errors(Y), case["cholesky_errors_" + tag]) < 1e-9
        assert rel(d.md_squared(Y), case["md_squared_" + tag]) < 1e-9
        assert rel(d.pivoted_cholesky_errors(Y), case["pivoted_cholesky_errors_" + tag]) < 1e-9
        assert rel(d.eigen_errors(Y), case["eigen_errors_" + tag]) < 1e-8
        assert np.shape(d.md_squared(Y)) == np.shape(case["md_squared_" + tag])
        assert np.shape(d.cholesky_errors(Y)) == Y.shape
    assert abs(d.kl(np.array(case["mean0"]), np.array(case["cov0"])) - case["kl"]) <= 1e-10 * max(1.0, abs(case["kl"]))
    if "samples5" in case:
        np.testing.assert_array_equal(d.samples(5), case["samples5"])
    G = gm.pivoted_cholesky(cov, backend="cpu")
    if "pivoted_cholesky" in case:
        np.testing.assert_allclose(G, case["pivoted_cholesky"], rtol=0, atol=1e-12 * np.abs(cov).max())
    piv = np.array(case["dpstrf_piv"])                  # G's rows in dpstrf's pivot order are lower triangular, and G G^T = cov
    assert np.all(np.triu(G[piv], 1) == 0)
    assert np.abs(G @ G.T - cov).max() <= 1e-12 * np.abs(cov).max()


def test_cpu_pivoted_cholesky_known_answers():
    for k in DATA["known"]:
        M = np.array(k["M"])
        np.testing.assert_allclose(gm.pivoted_cholesky(M, backend="cpu"), k["pivoted_cholesky"], rtol=1e-12, atol=1e-12)
        from gsum_amd._cpu import CpuContext
        ctx = CpuContext()
        info, piv = ctx.pstrf(ctx.upload(M))
        assert info == 0 and list(piv) == k["dpstrf_piv"]


def test_cpu_rank_deficient_raises_and_reports_rank():
    rd = DATA["rank_deficient"]
    assert rd["raises"]
    M = np.array(rd["M"])
    with pytest.raises(np.linalg.LinAlgError):
        gm.pivoted_cholesky(M, backend="cpu")
    from gsum_amd._cpu import CpuContext
    ctx = CpuContext()
    info, _ = ctx.pstrf(ctx.upload(M))
    assert info == rd["dpstrf_rank"] + 1
    with pytest.raises(np.linalg.LinAlgError):
        gm.Diagnostic(np.zeros(M.shape[0]), M, backend="cpu")


def test_cpu_shapes_and_misuse():
    c = CASES[1]
    mean, cov = np.array(c["mean"]), np.array(c["cov"])
    d = gm.Diagnostic(mean, cov, backend="cpu")
    n = mean.shape[0]
    assert d.cholesky_errors(mean).shape == (n,)
    assert np.ndim(d.md_squared(mean)) == 0 and d.md_squared(mean) == 0.0
    assert d.pivoted_cholesky_errors(np.zeros((n, 7)) + mean[:, None]).shape == (n, 7)
    assert d.samples(4, method="cholesky").shape == (n, 4)
    with pytest.raises(ValueError):
        d.samples(2, method="qr")
    with pytest.raises(ValueError):
        gm.Diagnostic(mean, cov, backend="tpu")
    from gsum_amd._cpu import CpuContext
    ctx = CpuContext()
    M = ctx.upload(cov)
    ctx.sqrt_errors(M, np.ones((n, 2)), pivot=False)
    with pytest.raises(ValueError):                   # the factor is unpivoted: a pivoted call is refused
        ctx.sqrt_errors(M, np.ones((n, 2)), pivot=True)


def test_eigen_errors_needs_the_cpu_backend():
    c = CASES[0]
    d = gm.Diagnostic.__new__(gm.Diagnostic)
    d.backend, d.cov, d.mean, d._eig = "hip", np.array(c["cov"]), np.array(c["mean"]), None
    with pytest.raises(NotImplementedError):
        d.eigen_errors(np.array(c["Y1"]))
