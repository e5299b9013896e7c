"""What tests/test_pointwise_cpu.py and tests/test_gpu_pointwise.py share: the fixture tests/golden/pointwise.json decoded, the models
of its cases rebuilt on a backend, and the magnitude M that the log-likelihood bound is relative to."""
import base64

import numpy as np
from scipy.special import loggamma

from conftest import load_golden

import gsum_amd as gm

LOGLIKE_RTOL = 1e-13          # times M: per-point terms carry a few ulps and a sum of n of them about log2(n) more, which stays below
#                               3e-15 * M at n = 2^20; float64 sat within 4e-16 * M of long-double truth at n = 350, 8192 and 2^20 with
#                               powers by pow or by repeated multiplication alike.  1e-13 leaves about 30x.


def D(v):
    return np.frombuffer(base64.b64decode(v["f64"]), "<f8").reshape(v["shape"]).copy()


def unwrap(a):
    """a stored ratio / ref as what was passed to the reference: a Python float for a 0-d entry, else the array"""
    a = D(a)
    return float(a) if a.ndim == 0 else a


def golden():
    return load_golden("pointwise.json")


def fit_model(rec, orders, excluded, backend, ratio=None):
    """the model of a fixture record fitted on a backend (``ratio``: where the record stores none)"""
    m = gm.TruncationPointwise(df=rec["df"], scale=rec["scale"], excluded=excluded, backend=backend)
    return m.fit(D(rec["y"]), ratio=unwrap(rec["ratio"]) if ratio is None else ratio, ref=unwrap(rec["ref"]), orders=np.asarray(orders))


def loglike_magnitude(model, ratio, ref):
    """M: the sum of the absolute values of the three groups of terms of log_likelihood(ratio, ref): the constants, the halves of
    df * log(df * scale_i^2 / 2) over the points, and the change-of-variables terms over what ratio and ref broadcast to."""
    ratio = model.ratio_ if ratio is None else ratio
    ref = model.ref_ if ref is None else ref
    df0, scale0 = model.df0, model.scale0
    mask = model.orders_mask_
    c = gm.coefficients(model.y_, ratio=ratio, ref=ref, orders=model.orders_)[:, mask]
    df = df0 + c.shape[1]
    consts = abs(loggamma(df / 2.)) + abs(0.5 * c.shape[1] * np.log(2 * np.pi))
    if df0 > 0:
        consts += abs(0.5 * df0 * np.log(df0 * scale0 ** 2 / 2.)) + abs(loggamma(df0 / 2.))
    points = np.sum(np.abs(0.5 * df * np.log((df0 * scale0 ** 2 + np.sum(c ** 2, axis=1)) / 2.)))
    jacobian = np.sum(np.abs(np.log(np.abs(ref)) + np.sum(model.orders_[mask]) * np.log(ratio)))
    return float(consts + points + jacobian)


def random_problem(n, k=6, seed=0, excluded=(0,)):
    """Seeded partial sums at n points and orders 0..k-1 with (n,) ratio and ref, for the hip-against-cpu comparisons."""
    rng = np.random.RandomState(seed + n)
    x = np.linspace(0, 1, n) if n > 1 else np.array([0.5])
    ratio, ref = 0.25 + 0.2 * x, 1.5 + np.cos(3 * x)
    orders = np.arange(k)
    y = gm.partials(rng.standard_normal((n, k)), ratio=ratio, ref=ref, orders=orders)
    return y, ratio, ref, orders, list(excluded)


# ---- the fixture's cases on a backend: every function asserts its bounds and returns what it achieved ------------------------------

def _rel(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))) if want.size else 0.0


def check_poc(g, backend):
    rec = g["poc"]
    y = D(rec["y"])
    m = gm.TruncationPointwise(df=rec["df"], backend=backend).fit(y=y, ratio=rec["ratio"])
    worst = 0.0
    for name, dob in (("68", 0.68), ("95", 0.95)):
        lower, upper = m.interval(dob, orders=2)
        worst = max(worst, _rel([lower, upper], D(rec["interval" + name])), _rel(m.pdf(lower[:, None], orders=2), D(rec["pdf_heights" + name])))
    worst = max(worst, _rel(m.pdf(D(rec["delta"])[:, None, None] + y, orders=2), D(rec["pdfs"])))
    assert worst <= 1e-12, worst
    return dict(rel=worst)


def check_model(g, rec, backend):
    """a record of g['models']: fitted attributes bit-equal, the scipy calls to 1e-12, every log_likelihood to LOGLIKE_RTOL * M"""
    m = fit_model(rec, g["orders"], g["excluded"], backend)
    np.testing.assert_array_equal(m.coeffs_, D(rec["coeffs"]))
    np.testing.assert_array_equal(m.scale_, D(rec["scale_"]))
    assert m.df_ == rec["df_"]
    np.testing.assert_array_equal(m.orders_mask_, rec["orders_mask"])
    np.testing.assert_array_equal(np.broadcast_to(m.dist_.kwds["scale"], D(rec["dist_scale"]).shape), D(rec["dist_scale"]))
    np.testing.assert_array_equal(m.coeffs_dist_.kwds["scale"], D(rec["scale_"]))
    yq = D(rec["yq"])
    thin = max(_rel(m.interval([0.68, 0.95]), D(rec["interval_all"])), _rel(m.interval(0.9, orders=3), D(rec["interval_one"])),
               _rel(m.interval([0.5], orders=[2, 5]), D(rec["interval_two"])), _rel(m.pdf(yq), D(rec["pdf"])),
               _rel(m.logpdf(yq, orders=[3, 4]), D(rec["logpdf"])), _rel(m.std(), D(rec["std"])))
    assert thin <= 1e-12, thin
    worst = 0.0
    calls = [(None, None, rec["loglike_default"])] + [(unwrap(c["ratio"]), None if c["ref"] is None else unwrap(c["ref"]), c["value"])
                                                       for c in rec["loglike"]]
    for ratio, ref, want in calls:
        got = m.log_likelihood(ratio=ratio, ref=ref)
        err = abs(float(got) - want) / loglike_magnitude(m, ratio, ref)
        print(f"log_likelihood {backend} df0={rec['df']} fit=({rec['fit_ratio']},{rec['fit_ref']}) err/M={err:.3e}")
        worst = max(worst, err)
    assert worst <= LOGLIKE_RTOL, worst
    m.close()
    return dict(thin_rel=thin, loglike_err_over_M=worst)


def check_scan(g, backend):
    """the Lambda_b-style scan: per-row log_likelihood and the grid against the reference's rows, then the posterior's summaries"""
    rec = g["scan"]
    ratios, want = D(rec["ratios"]), D(rec["log_like"])
    m = fit_model(rec, rec["orders"], rec["excluded"], backend, ratio=ratios[0])
    grid = m.log_likelihood_grid(ratios)
    assert grid.shape == want.shape and grid.dtype == np.float64
    M = np.array([loglike_magnitude(m, r, None) for r in ratios])
    err_grid = float(np.max(np.abs(grid - want) / M))
    err_rows = float(np.max(np.abs(np.array([m.log_likelihood(ratio=r) for r in ratios]) - want) / M))
    print(f"scan {backend}: grid err/M={err_grid:.3e} rows err/M={err_rows:.3e}")
    assert max(err_grid, err_rows) <= LOGLIKE_RTOL, (err_grid, err_rows)
    Lb, post = D(rec["Lb"]), D(rec["posterior"])
    np.testing.assert_array_equal(gm.hpd_pdf(pdf=post, alpha=0.68, x=Lb), D(rec["hpd68"]))
    np.testing.assert_array_equal(gm.hpd_pdf(pdf=post, alpha=0.95, x=Lb), D(rec["hpd95"]))
    assert gm.median_pdf(pdf=post, x=Lb) == rec["median"]
    m.close()
    return dict(grid_err_over_M=err_grid, rows_err_over_M=err_rows)


def check_diagnostic(g, rec, backend):
    y, dobs = D(rec["y"]), D(rec["dobs"])
    m = gm.TruncationPointwise(df=rec["df"], scale=rec["scale"], excluded=g["excluded"], backend=backend)
    m.fit(y[:, :4], ratio=D(rec["ratio"]), ref=D(rec["ref"]), orders=np.arange(4))
    D_CI, bands = m.credible_diagnostic(data=y[:, 4], dobs=dobs, band_intervals=rec["band_intervals"], band_dobs=D(rec["band_dobs"]), beta=rec["beta"])
    np.testing.assert_array_equal(D_CI, D(rec["D_CI"]))
    np.testing.assert_array_equal(m.credible_diagnostic(data=y[:, 4], dobs=dobs), D(rec["D_CI_only"]))
    want = D(rec["bands"])
    if rec["beta"]:
        band_rel = _rel(bands, want)
        assert band_rel <= 1e-9, band_rel
    else:
        np.testing.assert_array_equal(bands, want)
        band_rel = 0.0
    m.close()
    return dict(band_rel=band_rel)
