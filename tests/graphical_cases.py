"""tests/golden/graphical.json decoded (see make_golden_graphical.py) and the comparison of a gsum_amd.GraphicalDiagnostic's data
accessors and plot methods with it; shared by test_graphical_cpu.py and test_gpu_refdist.py.

Bounds: ``samples``, the credible-interval coverages and their bands equal (integer counts over n; percentiles of identical inputs);
``q_theory`` 1e-14 relative; errors, sorted errors and QQ bands 1e-9 max|want|, the bound of the reference comparison of the
errors (test_gpu_diagnostics.py): order statistics and their convex combinations are 1-Lipschitz in the max norm of the errors."""
import base64
import json
import os

import numpy as np

from conftest import GOLDEN

KINDS = ("individual", "cholesky", "pivoted_cholesky", "eigen")
REL = 1e-9


def _dec(v):
    if isinstance(v, dict) and "f64" in v:
        return np.frombuffer(base64.b64decode(v["f64"]), "<f8").reshape(v["shape"]).copy()
    if isinstance(v, dict):
        return {k: _dec(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_dec(x) for x in v]
    return v


def _load():
    with open(os.path.join(GOLDEN, "graphical.json")) as f:
        data = _dec(json.load(f))
    with open(os.path.join(GOLDEN, "diagnostics.json")) as f:
        inputs = {c["name"]: c for c in _dec(json.load(f))["cases"]}
    for c in data["cases"]:
        src = inputs[c["name"]]
        n = c["n"]
        cov = np.zeros((n, n))
        cov[np.tril_indices(n)] = src["cov_tril"]
        c["cov"] = cov + np.tril(cov, -1).T
        c["mean"], c["data"] = src["mean"], src["Y3"]
    return data


DATA = _load()
CASES = DATA["cases"]
INTERVALS = DATA["intervals"]
BAND_PERC = tuple(DATA["band_perc"])


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    r = float(np.abs(got - want).max() / np.abs(want).max())
    assert r <= REL, (what, r)
    return r


def check_accessors(g, case, eigen):
    """every data accessor of g against the numbers the reference drew; returns the worst relative deviation of the error-derived
    arrays.  ``eigen``: include the eigen kind (backend='cpu')."""
    P = case["panels"]
    np.testing.assert_array_equal(g.samples, case["samples"])
    worst = 0.0
    for kind in KINDS if eigen else KINDS[:3]:
        err, (lo, hi) = g.error_data(kind)
        worst = max(worst, _close(err, P[kind + "_errors"]["err"], kind))
        assert [lo, hi] == P[kind + "_errors"]["sd_lines"]
        q_theory, srt, bands = g.qq_data(kind, BAND_PERC)
        want = P[kind + "_errors_qq"]
        np.testing.assert_allclose(q_theory, want["q_theory"], rtol=1e-14, atol=0)
        worst = max(worst, _close(srt, want["data_sorted"], kind + " sorted"))
        assert bands.shape == (len(BAND_PERC), 2, case["n"])
        scale = np.abs(want["bands"]).max()
        r = float(np.abs(bands - want["bands"]).max() / scale)
        assert r <= REL, (kind + " bands", r)
        worst = max(worst, r)
    dci, cb = g.credible_interval_data(INTERVALS, BAND_PERC)
    np.testing.assert_array_equal(dci, P["credible_interval"]["dci_data"])
    np.testing.assert_array_equal(cb, P["credible_interval"]["bands"])
    md, ref = g.md_data()
    worst = max(worst, _close(md, P["md_squared"]["md"], "md"))
    assert [float(ref.ppf(0.975)), float(ref.ppf(0.025))] == P["md_squared"]["bounds"]
    return worst


def new_axis():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.close("all")
    return plt.subplots()[1]


def band_of(coll, x):
    """(lower, upper) of a fill_between(x, lower, upper) PolyCollection (the vertex order make_golden_graphical.py documents)"""
    (path,) = coll.get_paths()
    v = path.vertices
    n = len(x)
    assert len(v) == 2 * n + 3
    return v[1:n + 1, 1], v[n + 2:2 * n + 2, 1][::-1]


def check_plots(g, case, eigen):
    """every plot method on a fresh Agg axis: the artist counts and titles the fixture records, and the drawn arrays within the
    bounds above"""
    P = case["panels"]
    for kind in KINDS if eigen else KINDS[:3]:
        want = P[kind + "_errors"]
        ax = getattr(g, kind + "_errors")(ax=new_axis())
        assert (len(ax.lines), len(ax.collections), ax.get_title()) == (want["lines"], want["collections"], want["title"])
        assert [ax.lines[1].get_ydata()[0], ax.lines[2].get_ydata()[0]] == want["sd_lines"]
        np.testing.assert_array_equal(ax.lines[3].get_xdata(), want["index"])
        _close(np.stack([ln.get_ydata() for ln in ax.lines[3:]], axis=1), want["err"], kind)
        want = P[kind + "_errors_qq"]
        ax = getattr(g, kind + "_errors_qq")(ax=new_axis())
        assert (len(ax.lines), len(ax.collections), ax.get_title()) == (want["lines"], want["collections"], want["title"])
        assert (ax.get_xlabel(), ax.get_ylabel()) == ("Theoretical Quantiles", "Empirical Quantiles")
        x = np.asarray(ax.lines[0].get_xdata())
        np.testing.assert_allclose(x, want["q_theory"], rtol=1e-14, atol=0)
        _close(np.stack([ln.get_ydata() for ln in ax.lines[:-1]], axis=1), want["data_sorted"], kind + " sorted")
        scale = np.abs(want["bands"]).max()
        for coll, i in zip(ax.collections, range(len(BAND_PERC) - 1, -1, -1)):            # widest band first
            lo, hi = band_of(coll, x)
            assert max(np.abs(lo - want["bands"][i, 0]).max(), np.abs(hi - want["bands"][i, 1]).max()) <= REL * scale
    want = P["credible_interval"]
    ax = g.credible_interval(INTERVALS, list(BAND_PERC), ax=new_axis())
    assert (len(ax.lines), len(ax.collections), ax.get_title()) == (want["lines"], want["collections"], want["title"])
    np.testing.assert_array_equal(np.stack([ln.get_ydata() for ln in ax.lines[1:]]), want["dci_data"])
    for coll, b in zip(ax.collections, want["bands"]):
        lo, hi = band_of(coll, INTERVALS)
        np.testing.assert_array_equal(lo, b[0])
        np.testing.assert_array_equal(hi, b[1])
    want = P["md_squared"]
    ax = g.md_squared(ax=new_axis())
    assert (len(ax.lines), len(ax.collections), ax.get_title()) == (want["lines"], want["collections"], want["title"])
    np.testing.assert_array_equal(ax.lines[0].get_xdata(), want["ref_x"])
    np.testing.assert_array_equal(ax.lines[0].get_ydata(), want["ref_pdf"])
    _close([ln.get_xdata()[0] for ln in ax.lines[3:]], want["md"], "md")
