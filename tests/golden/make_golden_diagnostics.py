#!/usr/bin/env python3
"""Generate tests/golden/diagnostics.json from the reference's own Diagnostic and helpers.pivoted_cholesky.

Runs ONLY where a checkout of the reference (buqeye/gsum) is available; the file it writes holds data only -- seeded inputs and the
reference's outputs.  Usage:  GSUM_REFERENCE=<checkout of buqeye/gsum> python tests/golden/make_golden_diagnostics.py

``import gsum`` needs docrep, seaborn and statsmodels' MVT, absent here: they are in-memory placeholder modules as in make_golden.py;
the MVT placeholder records mean / sigma / df (the reference builds one for ``df`` set; only ``samples`` would draw from it, and the
fixture does not call it there).  No numeric code is stubbed.
"""
import base64
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GSUM_REFERENCE", os.path.join(HERE, "..", "..", "..", "reference"))


class MVT:
    def __init__(self, mean, sigma, df):
        self.mean, self.sigma, self.df = mean, sigma, df


def _import_reference():
    d = types.ModuleType("docrep")

    class _DP:
        def __init__(self, *a, **k):
            pass

        def get_sectionsf(self, *a, **k):
            return lambda f: f

        def dedent(self, f):
            return f

    d.DocstringProcessor = _DP
    sys.modules["docrep"] = d
    sys.modules["seaborn"] = types.ModuleType("seaborn")
    for name in ("statsmodels", "statsmodels.sandbox", "statsmodels.sandbox.distributions",
                 "statsmodels.sandbox.distributions.mv_normal"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["statsmodels.sandbox.distributions.mv_normal"].MVT = MVT
    sys.path.insert(0, REF)
    import gsum  # noqa
    from gsum import diagnostics, helpers  # noqa
    return diagnostics, helpers


diagnostics, helpers = _import_reference()
from scipy.linalg.lapack import dpstrf  # noqa: E402
from sklearn.gaussian_process.kernels import RBF, Matern  # noqa: E402


def L(a):
    """an array as its float64 bytes (little-endian, base64) and shape: exact, and half the size of decimal text; tests decode it
    with np.frombuffer(base64.b64decode(v["f64"]), "<f8").reshape(v["shape"])"""
    a = np.array(a, dtype="<f8", order="C")           # (keeps 0-d shapes)
    return {"f64": base64.b64encode(a.tobytes()).decode(), "shape": list(a.shape)}


def covariances(rng):
    out = []
    X = np.sort(rng.uniform(0, 1, 5))[:, None]
    out.append(("rbf_n5", RBF(0.4)(X) + 1e-4 * np.eye(5), None))
    X = rng.uniform(0, 1, (25, 1))
    out.append(("rbf_n25", 2.0 * RBF(0.25)(X) + 1e-4 * np.eye(25), None))
    X = rng.uniform(0, 1, (16, 2))
    out.append(("matern52_n16", Matern(0.3, nu=2.5)(X) + 1e-4 * np.eye(16), None))
    X = rng.uniform(0, 1, (60, 1))
    out.append(("matern32_n60_df5", 1.5 * Matern(0.2, nu=1.5)(X) + 1e-4 * np.eye(60), 5))
    # a GP predictive covariance: 20 training points with noise, 30 new points
    Xt, Xs = rng.uniform(0, 1, (20, 1)), np.linspace(0, 1, 30)[:, None]
    k = RBF(0.15)
    Ktt = k(Xt) + 1e-2 * np.eye(20)
    pred = k(Xs) - k(Xs, Xt) @ np.linalg.solve(Ktt, k(Xt, Xs))
    pred = 0.5 * (pred + pred.T) + 1e-6 * np.eye(30)
    out.append(("gp_predictive_n30", pred, None))
    out.append(("gp_predictive_n30_df5", pred, 5))
    return out


def kl_cov0(cov):
    """the second distribution's covariance of the kl() check: elementwise arithmetic, rebuilt bit for bit by the tests"""
    return 1.3 * cov + 0.01 * np.diag(np.diag(cov))


def case(name, cov, df, rng):
    n = cov.shape[0]
    assert np.linalg.cond(cov) <= 1e6, (name, np.linalg.cond(cov))
    mean = rng.normal(0, 0.5, n)
    Lc = np.linalg.cholesky(cov)
    Y3 = mean[:, None] + Lc @ rng.standard_normal((n, 3))
    Y1 = mean + Lc @ rng.standard_normal(n)
    d = diagnostics.Diagnostic(mean, cov, df=df, random_state=1)
    intervals = np.array([0.5, 0.68, 0.95])
    cov0 = kl_cov0(cov)
    mean0 = mean + 0.1 * rng.standard_normal(n)
    c, piv, rank, info = dpstrf(cov, tol=-1.0, lower=1)
    rec = dict(name=name, n=n, df=df, mean=L(mean), Y1=L(Y1), Y3=L(Y3), intervals=L(intervals), mean0=L(mean0),
               dpstrf_piv=[int(p) - 1 for p in piv], dpstrf_rank=int(rank), kl=float(d.kl(mean0, cov0)))
    if n <= 25:                 # (the larger cases are checked through dpstrf_piv: the fixture stays small)
        rec["pivoted_cholesky"] = L(helpers.pivoted_cholesky(cov))
    for tag, Y in (("1", Y1), ("3", Y3)):
        rec["individual_errors_" + tag] = L(d.individual_errors(Y))
        rec["chi2_" + tag] = L(d.chi2(Y))
        rec["cholesky_errors_" + tag] = L(d.cholesky_errors(Y))
        rec["md_squared_" + tag] = L(d.md_squared(Y))
        rec["pivoted_cholesky_errors_" + tag] = L(d.pivoted_cholesky_errors(Y))
        rec["eigen_errors_" + tag] = L(d.eigen_errors(Y))
        rec["credible_interval_" + tag] = L(d.credible_interval(Y, intervals))
    if df is None:
        rec["samples5"] = L(d.samples(5))
    return rec


def main():
    rng = np.random.RandomState(20261016)
    cases, covs = [], {}
    for name, cov, df in covariances(rng):
        cases.append(case(name, cov, df, rng))
        same = [k for k, v in covs.items() if v.shape == cov.shape and np.array_equal(v, cov)]
        if same:
            cases[-1]["cov_of"] = same[0]        # one covariance, two cases (df None / 5): stored once
        else:
            covs[name] = cov
            assert np.array_equal(cov, cov.T)
            cases[-1]["cov_tril"] = L(cov[np.tril_indices(cov.shape[0])])      # (exactly symmetric: the lower triangle, row by row)
    # the reference's known-answer inputs (gsum/tests/test.py:75-122): M = L L^T of three lower-triangular matrices
    lowers = [
        [[7., 0, 0, 0, 0, 0], [9, 13, 0, 0, 0, 0], [4, 10, 6, 0, 0, 0], [18, 1, 2, 14, 0, 0], [5, 11, 20, 3, 17, 0], [19, 12, 16, 15, 8, 21]],
        [[1, 0, 0], [2, 3, 0], [4, 5, 6.]],
        [[6, 0, 0], [3, 2, 0], [4, 1, 5.]],
    ]
    known = []
    for Lk in lowers:
        Lk = np.array(Lk)
        M = Lk @ Lk.T
        c, piv, rank, info = dpstrf(M, tol=-1.0, lower=1)
        known.append(dict(M=L(M), pivoted_cholesky=L(helpers.pivoted_cholesky(M)), dpstrf_piv=[int(p) - 1 for p in piv]))
    # rank deficient: 12 points of which 4 repeat exactly, no nugget
    X = np.arange(8.0)[:, None]
    X = np.vstack([X, X[:4]])
    Mr = RBF(0.5)(X)
    try:
        helpers.pivoted_cholesky(Mr)
        raised = False
    except np.linalg.LinAlgError:
        raised = True
    c, piv, rank, info = dpstrf(Mr, tol=-1.0, lower=1)
    rank_deficient = dict(M=L(Mr), raises=raised, dpstrf_rank=int(rank), dpstrf_info=int(info))
    out = dict(cases=cases, known=known, rank_deficient=rank_deficient)
    path = os.path.join(HERE, "diagnostics.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
