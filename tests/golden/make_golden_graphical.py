#!/usr/bin/env python3
"""Generate tests/golden/graphical.json from the reference's own GraphicalDiagnostic.

Runs ONLY where a checkout of the reference (buqeye/gsum) is available; the file it writes holds data only -- the reference's
sampled curves and the numbers of the artists its plot methods drew.
Usage:  GSUM_REFERENCE=<checkout of buqeye/gsum> python tests/golden/make_golden_graphical.py

The inputs are those of tests/golden/diagnostics.json (its df=None cases: covariance, mean and the three data curves Y3), read from
that file and not stored again.  The reference's GraphicalDiagnostic is built under the Agg backend with nref = 200; every panel
method draws on a fresh axis and the numbers are read back from the artists: the data of the lines, and the vertices of the
PolyCollections that fill_between made for the bands.  ``import gsum`` needs docrep, seaborn and statsmodels' MVT, absent here: they
are in-memory placeholder modules as in make_golden_diagnostics.py.  ``matplotlib.cm.get_cmap``, which the reference's
credible_interval calls and current matplotlib no longer has, is given a one-line stand-in.  No numeric code is stubbed.
"""
import base64
import json
import os
import sys
import types

import matplotlib
matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GSUM_REFERENCE", os.path.join(HERE, "..", "..", "..", "reference"))
NREF = 200
INTERVALS = np.linspace(0, 1, 21)
BAND_PERC = [0.68, 0.95]
KINDS = ("individual", "cholesky", "pivoted_cholesky", "eigen")


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
    if not hasattr(matplotlib.cm, "get_cmap"):
        matplotlib.cm.get_cmap = lambda name: matplotlib.colormaps[name]
    sys.path.insert(0, REF)
    import gsum  # noqa
    from gsum import diagnostics  # noqa
    return diagnostics


diagnostics = _import_reference()


def L(a):
    """an array as its float64 bytes (little-endian, base64) and shape, as in make_golden_diagnostics.py"""
    a = np.array(a, dtype="<f8", order="C")
    return {"f64": base64.b64encode(a.tobytes()).decode(), "shape": list(a.shape)}


def D(v):
    return np.frombuffer(base64.b64decode(v["f64"]), "<f8").reshape(v["shape"]).copy()


def band_of(coll, x):
    """(lower, upper) of a fill_between(x, lower, upper) PolyCollection: its one path runs (x0, upper0), the lower curve left to
    right, (x_last, upper_last), the upper curve right to left, and closes"""
    (path,) = coll.get_paths()
    v = path.vertices
    n = len(x)
    assert len(v) == 2 * n + 3, (len(v), n)
    assert np.array_equal(v[1:n + 1, 0], x) and np.array_equal(v[n + 2:2 * n + 2, 0], x[::-1])
    return v[1:n + 1, 1].copy(), v[n + 2:2 * n + 2, 1][::-1].copy()


def fresh():
    plt.close("all")
    return plt.subplots()[1]


def counts(ax):
    return dict(lines=len(ax.lines), collections=len(ax.collections))


def case(c, cov):
    n = c["n"]
    mean, data = D(c["mean"]), D(c["Y3"])
    g = diagnostics.GraphicalDiagnostic(data, mean, cov, df=None, random_state=1, nref=NREF)
    rec = dict(name=c["name"], n=n, nref=NREF, samples=L(g.samples), panels={})
    for kind in KINDS:
        ax = getattr(g, kind + "_errors")(ax=fresh())
        lines = ax.lines                                     # 0, -2 sd, +2 sd, then one line of markers per curve
        err = np.stack([ln.get_ydata() for ln in lines[3:]], axis=1)
        rec["panels"][kind + "_errors"] = dict(counts(ax), err=L(err), sd_lines=[float(lines[1].get_ydata()[0]), float(lines[2].get_ydata()[0])],
                                               index=L(lines[3].get_xdata()), title=ax.get_title())
        ax = getattr(g, kind + "_errors_qq")(ax=fresh())
        q_theory = np.asarray(ax.lines[0].get_xdata())
        srt = np.stack([ln.get_ydata() for ln in ax.lines[:-1]], axis=1)          # the last line is the diagonal
        bands = np.zeros((len(BAND_PERC), 2, n))
        for coll, i in zip(ax.collections, range(len(BAND_PERC) - 1, -1, -1)):    # drawn widest band first
            bands[i] = band_of(coll, q_theory)
        rec["panels"][kind + "_errors_qq"] = dict(counts(ax), q_theory=L(q_theory), data_sorted=L(srt), bands=L(bands), title=ax.get_title())
    ax = g.credible_interval(INTERVALS, BAND_PERC, ax=fresh())
    dci = np.stack([ln.get_ydata() for ln in ax.lines[1:]])                       # the first line is the diagonal
    bands = np.stack([np.stack(band_of(coll, INTERVALS)) for coll in ax.collections])
    rec["panels"]["credible_interval"] = dict(counts(ax), dci_data=L(dci), bands=L(bands), title=ax.get_title())
    ax = g.md_squared(ax=fresh())
    lines = ax.lines                                         # the reference pdf, its two 2 sigma lines, one vertical line per curve
    rec["panels"]["md_squared"] = dict(counts(ax), ref_x=L(lines[0].get_xdata()), ref_pdf=L(lines[0].get_ydata()),
                                       bounds=[float(lines[1].get_xdata()[0]), float(lines[2].get_xdata()[0])],
                                       md=L([ln.get_xdata()[0] for ln in lines[3:]]), title=ax.get_title())
    plt.close("all")
    return rec


def main():
    with open(os.path.join(HERE, "diagnostics.json")) as f:
        diag = json.load(f)
    cases = []
    for c in diag["cases"]:
        if c["df"] is not None or "cov_tril" not in c:
            continue
        cov = np.zeros((c["n"], c["n"]))
        cov[np.tril_indices(c["n"])] = D(c["cov_tril"])
        cov = cov + np.tril(cov, -1).T
        cases.append(case(c, cov))
    out = dict(inputs="diagnostics.json: cov_tril, mean, Y3 of the case of the same name", intervals=L(INTERVALS), band_perc=BAND_PERC,
               cases=cases)
    path = os.path.join(HERE, "graphical.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
