#!/usr/bin/env python3
"""Generate tests/golden/pointwise.json from the reference's own TruncationPointwise and helpers.

Runs ONLY where a checkout of the reference (buqeye/gsum) is available; the file it writes holds data only: seeded inputs and the
numbers the reference returned for them.
Usage:  GSUM_REFERENCE=<checkout of buqeye/gsum> python tests/golden/make_golden_pointwise.py

Inputs: ``partials`` of standard normal coefficients from ``RandomState(seed)``, with a ratio and a reference scale that are scalars
or smooth (n,) arrays; every input is stored with its case.  ``import gsum`` needs docrep, seaborn and statsmodels' MVT, absent here:
they are in-memory placeholder modules as in make_golden_diagnostics.py.  ``numpy.trapz``, which the reference's ``hpd_pdf`` and
``median_pdf`` call, is bound to ``numpy.trapezoid`` when the installed numpy has only the latter.  No numeric code is stubbed, and
no case had to be left out.

Cases
  poc         the three rows of the truncation_recap notebook's proof of concept (df = 0, Q = 0.33): interval(0.68 / 0.95, orders=2),
              pdf at the lower bounds and on a grid of y
  models      n = 8 points, orders [0, 2, 3, 4, 5] with excluded = [0], the priors (df, scale) in {(0, 1), (0.6, 0.8), (1, 1)}, and
              scalar / array ratio x scalar / array ref at fit: the fitted attributes, interval, pdf, logpdf, std, and
              log_likelihood for scalar / array ratio x scalar / array ref arguments (and the defaults)
  scan        a breakdown-scale style scan: 64 rows of (n,) ratios Q_i(Lambda) = p_i / Lambda, log_likelihood per row, the posterior
              on the Lambda grid with its hpd_pdf (0.68, 0.95) and median_pdf
  diagnostic  credible_diagnostic with beta = True and beta = False, dobs = arange(0.1, 1, 0.1), three band_intervals
  hpd         hpd(scipy.stats.beta, alpha, a, b) for two parameter sets
  cartesian   cartesian of two and of three arrays
"""
import base64
import json
import os
import sys
import types

import numpy as np
import scipy.stats

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GSUM_REFERENCE", os.path.join(HERE, "..", "..", "..", "reference"))
ORDERS = np.array([0, 2, 3, 4, 5])
EXCLUDED = [0]
PRIORS = [(0, 1), (0.6, 0.8), (1, 1)]
N = 8


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
    if not hasattr(np, "trapz"):
        np.trapz = np.trapezoid
    sys.path.insert(0, REF)
    import gsum  # noqa
    return gsum


gm = _import_reference()


def L(a):
    """an array as its float64 bytes (little-endian, base64) and shape, as in make_golden_diagnostics.py"""
    a = np.array(a, dtype="<f8", order="C")
    return {"f64": base64.b64encode(a.tobytes()).decode(), "shape": list(a.shape)}


def point_arrays(n):
    x = np.linspace(0, 1, n)
    return 0.25 + 0.2 * x, 1.5 + np.cos(3 * x)                  # a ratio in (0, 1) and a reference scale that changes sign nowhere


def make_y(seed, n, orders, ratio, ref):
    coeffs = np.random.RandomState(seed).standard_normal((n, len(orders)))
    return gm.partials(coeffs, ratio=ratio, ref=ref, orders=orders)


def poc():
    coeffs = np.array([[1.0, 1.0, 1.0], [1.0, 0.5, 0.1], [1.0, 0.1, 0.1]])
    y = gm.partials(coeffs, ratio=0.33)
    model = gm.TruncationPointwise(df=0).fit(y=y, ratio=0.33)
    rec = dict(y=L(y), ratio=0.33, df=0)
    for name, dob in (("68", 0.68), ("95", 0.95)):
        lower, upper = model.interval(dob, orders=2)
        rec["interval" + name] = L([lower, upper])
        rec["pdf_heights" + name] = L(model.pdf(lower[:, None], orders=2))
    delta = np.linspace(-0.15, 0.15, 25)
    rec["delta"] = L(delta)
    rec["pdfs"] = L(model.pdf(delta[:, None, None] + y, orders=2))
    return rec


def models():
    ratio_n, ref_n = point_arrays(N)
    out = []
    for pi, (df, scale) in enumerate(PRIORS):
        for fit_ratio in ("scalar", "array"):
            for fit_ref in ("scalar", "array"):
                ratio = 0.3 if fit_ratio == "scalar" else ratio_n
                ref = 2.5 if fit_ref == "scalar" else ref_n
                y = make_y(100 + pi, N, ORDERS, ratio, ref)
                m = gm.TruncationPointwise(df=df, scale=scale, excluded=EXCLUDED).fit(y, ratio=ratio, ref=ref, orders=ORDERS)
                yq = np.array([-0.3, 0.2])[:, None, None] + m.y_masked_
                rec = dict(df=df, scale=scale, fit_ratio=fit_ratio, fit_ref=fit_ref, y=L(y), ratio=L(ratio), ref=L(ref),
                           coeffs=L(m.coeffs_), df_=float(m.df_), scale_=L(m.scale_), dist_scale=L(np.broadcast_to(m.dist_.kwds["scale"], yq.shape[1:])),
                           orders_mask=[bool(b) for b in m.orders_mask_],
                           interval_all=L(m.interval([0.68, 0.95])), interval_one=L(m.interval(0.9, orders=3)),
                           interval_two=L(m.interval([0.5], orders=[2, 5])), yq=L(yq), pdf=L(m.pdf(yq)), logpdf=L(m.logpdf(yq, orders=[3, 4])),
                           std=L(m.std()), loglike_default=float(m.log_likelihood()), loglike=[])
                ratio2, ref2 = 0.8 * ratio_n + 0.05, 1.1 * ref_n
                for rk, rv in (("scalar", 0.41), ("array", ratio2)):
                    for fk, fv in (("scalar", 1.7), ("array", ref2), ("default", None)):
                        rec["loglike"].append(dict(ratio_kind=rk, ref_kind=fk, ratio=L(rv), ref=None if fv is None else L(fv),
                                                   value=float(m.log_likelihood(ratio=rv, ref=fv))))
                out.append(rec)
    return out


def scan():
    n, G = 8, 64
    p = np.linspace(120.0, 330.0, n)                             # momenta; Q_i = p_i / Lambda
    Lb = np.linspace(400.0, 1350.0, G)
    ref = 20.0 + 0.05 * p
    orders = np.array([0, 2, 3, 4, 5])
    y = make_y(7, n, orders, p / 600.0, ref)
    ratios = p[None, :] / Lb[:, None]
    m = gm.TruncationPointwise(df=0, excluded=[0]).fit(y, ratio=ratios[0], ref=ref, orders=orders)
    log_like = np.array([m.log_likelihood(ratio=r) for r in ratios])
    post = np.exp(log_like + np.log(1.0 / Lb) - np.max(log_like + np.log(1.0 / Lb)))
    post /= np.trapz(post, x=Lb)
    return dict(y=L(y), ref=L(ref), orders=[int(o) for o in orders], excluded=[0], df=0, scale=1, Lb=L(Lb), ratios=L(ratios), log_like=L(log_like),
                posterior=L(post), hpd68=L(gm.hpd_pdf(pdf=post, alpha=0.68, x=Lb)), hpd95=L(gm.hpd_pdf(pdf=post, alpha=0.95, x=Lb)),
                median=float(gm.median_pdf(pdf=post, x=Lb)))


def diagnostic():
    ratio_n, ref_n = point_arrays(24)
    y = make_y(11, 24, np.arange(5), ratio_n, ref_n)
    dobs = np.arange(0.1, 1, 0.1)
    band_dobs = np.linspace(0.001, 1, 12)
    band_intervals = [0.68, 0.95, 0.99]
    out = []
    for df, scale in ((0.6, 0.8), (1, 1)):
        m = gm.TruncationPointwise(df=df, scale=scale, excluded=EXCLUDED).fit(y[:, :4], ratio=ratio_n, ref=ref_n, orders=np.arange(4))
        for beta in (True, False):
            D_CI, bands = m.credible_diagnostic(data=y[:, 4], dobs=dobs, band_intervals=band_intervals, band_dobs=band_dobs, beta=beta)
            out.append(dict(df=df, scale=scale, beta=beta, y=L(y), ratio=L(ratio_n), ref=L(ref_n), dobs=L(dobs), band_dobs=L(band_dobs),
                            band_intervals=band_intervals, D_CI=L(D_CI), bands=L(bands), D_CI_only=L(m.credible_diagnostic(data=y[:, 4], dobs=dobs))))
    return out


def main():
    out = dict(orders=[int(o) for o in ORDERS], excluded=EXCLUDED, poc=poc(), models=models(), scan=scan(), diagnostic=diagnostic(),
               hpd=[dict(alpha=a, a=p, b=q, interval=L(gm.hpd(scipy.stats.beta, a, p, q))) for a, p, q in ((0.68, 7.0, 19.0), (0.95, 2.5, 1.2))],
               cartesian=[dict(arrays=[L(a) for a in arrs], product=L(gm.cartesian(*arrs)))
                          for arrs in ([np.array([96., 143, 200, 300]), np.array([60., 120])], [np.arange(3.), np.arange(2.), np.array([5., 7.])])])
    path = os.path.join(HERE, "pointwise.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
