"""gsum_amd.GraphicalDiagnostic on backend='cpu' against the numbers the reference's own GraphicalDiagnostic drew
(tests/golden/graphical.json, make_golden_graphical.py); bounds in graphical_cases.py."""
import subprocess
import sys

import numpy as np
import pytest
import scipy.stats as stats

from conftest import ROOT
from graphical_cases import CASES, INTERVALS, BAND_PERC, check_accessors, check_plots, new_axis

import gsum_amd as gm  # noqa: E402


def _make(case, **kw):
    return gm.GraphicalDiagnostic(case["data"], case["mean"], case["cov"], nref=case["nref"], backend="cpu", **kw)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cpu_accessors_match_reference(case):
    g = _make(case)
    assert g.data.shape == (case["n"], 3) and g.samples.shape == (case["n"], case["nref"])
    assert isinstance(g.diagnostic, gm.Diagnostic) and g.backend == "cpu"
    check_accessors(g, case, eigen=True)
    g.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cpu_plots_match_reference(case):
    pytest.importorskip("matplotlib")
    g = _make(case)
    check_plots(g, case, eigen=True)
    for name in ("box", "violin"):
        with pytest.raises(NotImplementedError, match="seaborn"):
            getattr(g, name)(np.zeros(3), np.zeros(10))
    with pytest.raises(NotImplementedError, match="seaborn"):
        g.md_squared(type="box")
    with pytest.raises(NotImplementedError):
        g.kl(None, None)
    with pytest.raises(NotImplementedError):
        g.plotzilla(None, gp=object())


def test_cpu_figures_and_remaining_panels():
    pytest.importorskip("matplotlib")
    import matplotlib.pyplot as plt
    case = CASES[1]
    g = _make(case)
    fig, axes = g.essentials(bare=True)
    assert len(axes) == 3
    assert [len(ax.lines) for ax in axes] == [6, 6, 4] and len(axes[2].collections) == 2      # every panel on its own axis
    fig, axes = g.essentials()
    assert axes.shape == (2, 3) and all(len(ax.lines) > 0 for ax in axes.ravel())
    fig, axes = g.essentials(eigen=False)
    assert not axes[0, 1].axison and not axes[1, 1].axison and len(axes[0, 1].lines) == 0
    fig, axes = g.plotzilla(None)
    assert axes.shape == (4, 3) and len(axes[1, 2].lines) == 6 and len(axes[0, 1].lines) == 0
    plt.close("all")
    # hist without an axis (the reference touches ax before its default), with a sampled reference and without vlines
    plt.figure()
    ax = g.hist(np.array([1.0, 2.0]), np.random.RandomState(0).standard_normal(50), vlines=False, title="t", xlabel="x", ylabel="y")
    assert ax is plt.gca() and (ax.get_title(), ax.get_xlabel(), ax.get_ylabel()) == ("t", "x", "y")
    # the general qq with a function of the caller's
    ax = g.qq(g.data, g.samples, [0.68, 0.95], g.diagnostic.cholesky_errors, title="q", ax=new_axis())
    assert len(ax.lines) == 4 and len(ax.collections) == 2 and ax.get_title() == "q"
    # variogram: a float bin count in the reference; here it draws three lines per curve
    X = np.linspace(0, 1, case["n"])[:, None]
    ax = g.variogram(X, ax=new_axis())
    assert len(ax.lines) == 9 and ax.get_title() == "Variogram" and ax.get_xlabel() == "Lag"
    plt.close("all")
    g.close()


def test_one_dimensional_data_and_styles():
    case = CASES[0]
    g = gm.GraphicalDiagnostic(case["data"][:, 0], case["mean"], case["cov"], nref=7, colors=["r"], markers=["s"], labels=["a"],
                               markeredgecolors=["k"], markerfillstyles=["none"], backend="cpu")
    assert g.data.shape == (case["n"], 1) and g.samples.shape == (case["n"], 7)
    q, srt, bands = g.qq_data("cholesky", band_perc=(0.5,))
    assert srt.shape == (case["n"], 1) and bands.shape == (1, 2, case["n"]) and np.all(bands[0, 0] <= bands[0, 1])
    with pytest.raises(ValueError):
        g.qq_data("svd")
    pytest.importorskip("matplotlib")
    ax = g.cholesky_errors(ax=new_axis())
    assert ax.lines[3].get_marker() == "s" and ax.lines[3].get_color() == "r"


def test_student_t_properties():
    """df set: the reference samples from statsmodels' MVT (not available to the fixture generator), so this is a property test"""
    case = CASES[2]
    n, df = case["n"], 5
    g = gm.GraphicalDiagnostic(case["data"], case["mean"], case["cov"], df=df, nref=40, backend="cpu")
    assert g.samples.shape == (n, 40) and np.all(np.isfinite(g.samples))
    ref = g.md_ref_dist
    want = stats.f(dfn=n, dfd=df, scale=(df - 2) * n / df)
    assert ref.dist.name == "f" and ref.args == want.args and ref.kwds == want.kwds
    q_theory, srt, bands = g.qq_data("pivoted_cholesky")
    np.testing.assert_array_equal(q_theory, stats.t(df=df).ppf((np.arange(1, n + 1) - 0.5) / n))
    assert srt.shape == (n, 3) and bands.shape == (2, 2, n) and np.all(np.isfinite(srt)) and np.all(np.isfinite(bands))
    assert np.all(np.diff(srt, axis=0) >= 0) and np.all(bands[1, 0] <= bands[0, 0]) and np.all(bands[0, 1] <= bands[1, 1])
    dci, cb = g.credible_interval_data(INTERVALS, BAND_PERC)
    assert dci.shape == (3, len(INTERVALS)) and cb.shape == (2, 2, len(INTERVALS)) and np.all((dci >= 0) & (dci <= 1))
    err, (lo, hi) = g.error_data("individual")
    assert hi == 2 * stats.t(df=df).std() and lo == -hi and err.shape == (n, 3)
    md, _ = g.md_data()
    assert md.shape == (3,) and np.all(md > 0)
    g.close()


_NO_MATPLOTLIB = r"""
import importlib.abc, sys
class Block(importlib.abc.MetaPathFinder):
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in ("matplotlib", "cycler"):
            raise ImportError("masked: " + name)
sys.meta_path.insert(0, Block())
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import gsum_amd as gm
assert "matplotlib" not in sys.modules
from graphical_cases import CASES, check_accessors
case = CASES[0]
g = gm.GraphicalDiagnostic(case["data"], case["mean"], case["cov"], nref=case["nref"], backend="cpu")
check_accessors(g, case, eigen=True)
try:
    g.essentials(bare=True)
except ImportError:
    pass
else:
    raise SystemExit("a plot method ran without matplotlib")
assert "matplotlib" not in sys.modules
print("ok")
"""


def test_no_matplotlib_needed_for_import_and_accessors():
    out = subprocess.run([sys.executable, "-c", _NO_MATPLOTLIB, ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
