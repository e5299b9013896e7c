"""The device pivoted Cholesky (gsum_sqrt_errors, pivot = 1) against LAPACK dpstrf, many-column errors against scipy, and
gsum_amd.Diagnostic on backend='hip' against the reference's outputs (tests/golden/diagnostics.json)."""
import base64
import json
import os

import numpy as np
import pytest
from scipy.linalg import solve_triangular
from scipy.linalg.lapack import dpstrf
from sklearn.gaussian_process.kernels import RBF, Matern

from conftest import GOLDEN, record_parity

pytestmark = pytest.mark.gpu

import gsum_amd as gm  # noqa: E402
from gsum_amd import _lib  # noqa: E402


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


@pytest.fixture(scope="module")
def ctx():
    return gm.default_context()


def _spd(n, seed):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (n, 2))
    return Matern(0.3, nu=2.5)(X) + 1e-3 * np.eye(n)


def _gaps_and_choice(A, L, piv, steps):
    """per step j < steps of a pivoted factor (L in pivot order, piv): the updated diagonal of every candidate i >= j; returns the
    relative gap between the best and second-best candidate and the chosen candidate's value over the best one"""
    n = A.shape[0]
    d0 = np.diag(A)[piv]
    gaps, ratio = np.ones(steps), np.ones(steps)
    acc = np.zeros(n)
    for j in range(steps):
        upd = d0[j:] - acc[j:]
        best = upd.max()
        ratio[j] = upd[0] / best
        if n - j > 1:
            srt = np.sort(upd)[::-1]
            gaps[j] = (srt[0] - srt[1]) / abs(srt[0])
        acc += L[:, j] ** 2
    return gaps, ratio


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 2048, 8192])
def test_pstrf_against_lapack(ctx, n):
    A = _spd(n, n)
    M = ctx.upload(A)
    try:
        info, piv = ctx.pstrf(M)
        assert info == 0
        Lg = M.to_host()
    finally:
        M.free()
    assert sorted(piv.tolist()) == list(range(n))
    assert np.all(np.triu(Lg, 1) == 0)
    rec = np.abs(A[np.ix_(piv, piv)] - Lg @ Lg.T).max() / np.abs(A).max()
    assert rec <= 1e-12, rec
    c, lp, rank, linfo = dpstrf(A, tol=-1.0, lower=1)
    lp = lp.astype(np.int64) - 1
    assert rank == n and linfo == 0
    steps = n if n <= 2048 else 512         # (the host walk is O(n) per step)
    gaps, _ = _gaps_and_choice(A, np.tril(c), lp, steps)
    _, ratio = _gaps_and_choice(A, Lg, piv, steps)
    assert ratio.min() >= 1 - 1e-12, ratio.min()
    same = 0
    for j in range(steps):
        # step 0 ties exactly on a constant diagonal and both take the first index (MAXLOC); later, a gap of 1e-10 or less is a
        # near-tie the two rounding histories may resolve differently, and the orders part there
        if j > 0 and gaps[j] <= 1e-10:
            break
        assert piv[j] == lp[j], (j, piv[j], lp[j])
        same += 1
    record_parity(f"pstrf_n{n}", reconstruction=float(rec), pivots_equal_before_first_near_tie=same)


@pytest.mark.parametrize("kind", ["xxt", "duplicates"])
def test_pstrf_rank_deficient_matches_lapack(ctx, kind):
    rng = np.random.RandomState(7)
    if kind == "xxt":
        X = rng.standard_normal((300, 12))
        A = X @ X.T
    else:
        P = np.arange(50.0)[:, None]
        A = RBF(0.5)(np.vstack([P, P[:30]]))
    c, lp, rank, linfo = dpstrf(A, tol=-1.0, lower=1)
    assert linfo == 1
    M = ctx.upload(A)
    try:
        info, piv = ctx.pstrf(M)
        assert info == rank + 1, (info, rank)
        assert not M.factored
        np.testing.assert_array_equal(M.to_host(), A)       # a rank-deficient search leaves the matrix as it was
    finally:
        M.free()
    with pytest.raises(np.linalg.LinAlgError):
        gm.pivoted_cholesky(A)


def test_errors_many_columns_n8192(ctx):
    n = 8192
    rng = np.random.RandomState(3)
    X = np.sort(rng.uniform(0, 10, n))[:, None]
    A = RBF(0.5)(X) + 1e-2 * np.eye(n)
    mean = rng.standard_normal(n)
    Lh = np.linalg.cholesky(A)
    Yall = mean[:, None] + Lh @ rng.standard_normal((n, 1000))
    F = ctx.upload(A)
    P = ctx.upload(A)
    try:
        ctx.sqrt_errors(F, Yall[:, :1], mean, pivot=False)            # factorises F (potrf)
        info, piv = ctx.pstrf(P)
        assert info == 0
        Lp = np.linalg.cholesky(A[np.ix_(piv, piv)])
        worst = 0.0
        for k in (0, 1, 16, 17, 1000):
            Y = Yall[:, :k]
            E, m2 = ctx.sqrt_errors(F, Y, mean, pivot=False, md2=True)
            Ep, m2p = ctx.sqrt_errors(P, Y, mean, pivot=True, md2=True)
            assert E.shape == (n, k) and m2.shape == (k,)
            if k == 0:
                continue
            R = Y - mean[:, None]
            Eh = solve_triangular(Lh, R, lower=True)
            Eph = solve_triangular(Lp, R[piv], lower=True)
            r1 = np.abs(E - Eh).max() / np.abs(Eh).max()
            r2 = np.abs(Ep - Eph).max() / np.abs(Eph).max()
            r3 = np.abs(m2 - m2p).max() / np.abs(m2).max()
            r4 = np.abs(m2 - (Eh ** 2).sum(0)).max() / np.abs(m2).max()
            assert max(r1, r2, r3, r4) <= 1e-10, (k, r1, r2, r3, r4)
            worst = max(worst, r1, r2, r3, r4)
        with pytest.raises(ValueError):                                # the plain factor refuses a pivoted call and vice versa
            ctx.sqrt_errors(F, Yall[:, :2], mean, pivot=True)
        with pytest.raises(ValueError):
            ctx.sqrt_errors(P, Yall[:, :2], mean, pivot=False)
    finally:
        F.free()
        P.free()
    record_parity("sqrt_errors_n8192", worst_rel=worst)


@pytest.mark.parametrize("case", DATA["cases"], ids=[c["name"] for c in DATA["cases"]])
def test_hip_diagnostic_matches_reference(case):
    mean, cov = np.array(case["mean"]), np.array(case["cov"])
    d = gm.Diagnostic(mean, cov, df=case["df"], random_state=1, backend="hip")
    worst = 0.0
    try:
        for tag in ("1", "3"):
            Y = np.array(case["Y" + tag])
            np.testing.assert_array_equal(d.individual_errors(Y), case["individual_errors_" + tag])
            np.testing.assert_array_equal(d.chi2(Y), case["chi2_" + tag])
            np.testing.assert_array_equal(d.credible_interval(Y, np.array(case["intervals"])), case["credible_interval_" + tag])
            for name in ("cholesky_errors", "md_squared", "pivoted_cholesky_errors"):
                got, want = np.asarray(getattr(d, name)(Y)), np.asarray(case[name + "_" + tag])
                assert got.shape == want.shape, name
                r = float(np.abs(got - want).max() / np.abs(want).max())
                assert r <= 1e-9, (name, tag, r)
                worst = max(worst, r)
        with pytest.raises(NotImplementedError):
            d.eigen_errors(np.array(case["Y1"]))
        kl = d.kl(np.array(case["mean0"]), np.array(case["cov0"]))
        rk = abs(kl - case["kl"]) / max(1.0, abs(case["kl"]))
        assert rk <= 1e-10, rk
        if "samples5" in case:
            np.testing.assert_array_equal(d.samples(5), case["samples5"])
        if case["df"] is not None:
            s = d.samples(3)
            assert s.shape == (case["n"], 3) and np.all(np.isfinite(s))
    finally:
        d.close()
    G = gm.pivoted_cholesky(cov)
    if "pivoted_cholesky" in case:
        rg = float(np.abs(G - np.array(case["pivoted_cholesky"])).max() / np.abs(cov).max())
    else:                                               # (larger cases: dpstrf's pivots and the reconstruction)
        piv = np.array(case["dpstrf_piv"])
        assert np.all(np.triu(G[piv], 1) == 0)
        rg = float(np.abs(G @ G.T - cov).max() / np.abs(cov).max())
    assert rg <= 1e-12, rg
    record_parity(f"diagnostic_{case['name']}", worst_rel=worst, kl_rel=float(rk), pivoted_cholesky=rg)


def test_hip_known_answers_and_rank_deficient():
    for k in DATA["known"]:
        M = np.array(k["M"])
        np.testing.assert_allclose(gm.pivoted_cholesky(M), k["pivoted_cholesky"], rtol=1e-12, atol=1e-12 * np.abs(M).max())
    with pytest.raises(np.linalg.LinAlgError):
        gm.pivoted_cholesky(np.array(DATA["rank_deficient"]["M"]))
    ctx = gm.default_context()
    M = ctx.upload(np.array(DATA["rank_deficient"]["M"]))
    try:
        assert ctx.pstrf(M)[0] == DATA["rank_deficient"]["dpstrf_rank"] + 1
    finally:
        M.free()


def test_diagnostic_8192_points_1000_curves():
    n = 8192
    rng = np.random.RandomState(11)
    X = np.sort(rng.uniform(0, 20, n))[:, None]
    cov = RBF(1.0)(X) + 1e-2 * np.eye(n)
    mean = rng.standard_normal(n)
    Y = mean[:, None] + np.linalg.cholesky(cov) @ rng.standard_normal((n, 1000))
    d = gm.Diagnostic(mean, cov)
    try:
        md2 = d.md_squared(Y)
        Ep = d.pivoted_cholesky_errors(Y)
    finally:
        d.close()
    want = (solve_triangular(np.linalg.cholesky(cov), Y - mean[:, None], lower=True) ** 2).sum(0)
    r = np.abs(md2 - want).max() / want.max()
    assert r <= 1e-10, r
    assert Ep.shape == (n, 1000)
    assert np.abs((Ep ** 2).sum(0) - want).max() / want.max() <= 1e-10


def test_predict_unchanged_by_a_diagnostic(ctx):
    n, m = 2048, 300
    rng = np.random.RandomState(5)
    X = np.sort(rng.uniform(0, 10, n))[:, None]
    Xs = np.linspace(0, 10, m)[:, None]
    rhs = rng.standard_normal((n, 3))
    desc = gm.describe_kernel(RBF(0.7), 1)
    def run():
        L, info = ctx.factorize(desc, X, diag_add=1e-6)
        try:
            assert info == 0
            return ctx.predict_terms(L, desc, X, Xs, rhs=rhs, want_cov=True)
        finally:
            L.free()
    before = run()
    d = gm.Diagnostic(np.zeros(n), RBF(0.7)(X) + 1e-6 * np.eye(n))
    d.md_squared(rng.standard_normal((n, 40)))
    d.pivoted_cholesky_errors(rng.standard_normal((n, 40)))
    d.close()
    after = run()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
