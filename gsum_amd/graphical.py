"""``GraphicalDiagnostic`` (gsum/diagnostics.py:197-669): the diagnostics of some data beside their reference distributions.

The reference distributions are made by simulation: ``nref`` curves are drawn from the model, pushed through the same diagnostic as
the data, and shown as percentile bands.  The errors of the curves come from the owned ``Diagnostic`` (device factors); the stage
after them -- sort along the points, percentiles across the curves, credible-interval coverages -- runs in libgsum_refdist.so
(refdist.py) on ``backend='hip'`` and as the reference's numpy expressions on ``backend='cpu'``.

Two layers.  The data accessors (``qq_data``, ``credible_interval_data``, ``error_data``, ``md_data``) return the numbers of a panel
and never import matplotlib; the plot methods carry the reference's names, arguments, titles, labels and artist order, import
matplotlib when called and draw those numbers.

Where the reference cannot be carried over literally:

* ``matplotlib.cm.get_cmap`` is gone from current matplotlib: ``credible_interval`` takes ``matplotlib.colormaps['Greys']``.
* ``hist`` draws on ``ax`` before its ``ax is None`` default in the reference; here the default is resolved first.
* ``variogram`` gives ``np.linspace`` a float bin count in the reference; here ``int(nbins)``, and the curves go to the variogram
  one per row (``data.T``).
* ``essentials`` and ``plotzilla`` hand each panel its axis as the first positional argument in the reference, where the panel
  methods take ``title`` first; here it is passed as ``ax=``, so every panel lands on its own axis.
* ``box``, ``violin`` and ``md_squared(type='box')`` need seaborn's swarm plot: they raise NotImplementedError naming seaborn.
* ``kl`` iterates over the points axis of ``samples`` in the reference and has no well-defined behaviour to port: it raises
  NotImplementedError, and so does ``plotzilla`` when given a ``gp``.
* The eigen panels need ``Diagnostic.eigen_errors``, which exists on ``backend='cpu'`` only.  ``qq_data('eigen')``,
  ``eigen_errors`` and ``eigen_errors_qq`` raise its NotImplementedError on 'hip'; ``essentials(bare=False)`` and ``plotzilla``
  take ``eigen=True`` and on 'hip' raise before drawing anything unless called with ``eigen=False``, which switches those axes off.
* The default colors, markers and fill styles come from matplotlib's property cycle and are resolved at the first plot call.
"""
from __future__ import annotations

import numpy as np
import scipy.stats as stats

from . import refdist
from .diagnostics import Diagnostic

__all__ = ["GraphicalDiagnostic"]

_KINDS = ("individual", "cholesky", "pivoted_cholesky", "eigen")
_DEFAULT_BANDS = (0.68, 0.95)
_EIGEN_MESSAGE = ("the eigen panels need Diagnostic.eigen_errors, which the device library does not provide: "
                  "call with eigen=False, or use backend='cpu'")

# The figures as tables: (grid position, panel method, needs the eigen errors).  Every panel method takes ``ax=``.
_ESSENTIALS = (((0, 0), "md_squared", False), ((1, 0), "_credible_interval_default", False),
               ((0, 1), "eigen_errors", True), ((1, 1), "eigen_errors_qq", True),
               ((0, 2), "pivoted_cholesky_errors", False), ((1, 2), "pivoted_cholesky_errors_qq", False))
_ESSENTIALS_BARE = ((0, "md_squared", "MD"), (1, "pivoted_cholesky_errors", "PC"), (2, "_credible_interval_default", "CI"))
_PLOTZILLA = (((0, 0), "md_squared", False), ((0, 2), "_credible_interval_default", False),
              ((1, 0), "individual_errors", False), ((2, 0), "individual_errors_qq", False),
              ((1, 1), "cholesky_errors", False), ((2, 1), "cholesky_errors_qq", False),
              ((1, 2), "eigen_errors", True), ((2, 2), "eigen_errors_qq", True),
              ((3, 0), "pivoted_cholesky_errors", False), ((3, 1), "pivoted_cholesky_errors_qq", False))


def _band_percentiles(band_perc):
    """(len(band_perc), 2): the lower and upper percentile of the central band holding a fraction b of the curves"""
    b = np.asarray(list(band_perc), dtype=float)
    return np.stack([100 * (1. - b) / 2, 100 * (1. + b) / 2], axis=1)


def _tag(name):
    return r"$\mathrm{D}_{\mathrm{%s}}$" % name


class GraphicalDiagnostic:
    R"""Plots of diagnostics and their reference distributions: gsum.diagnostics.GraphicalDiagnostic.

    data : (n_samples, [n_curves]); mean, cov, df, random_state : the owned ``Diagnostic``'s (``.diagnostic``);
    nref : reference curves drawn at construction (``.samples``, shape (n_samples, nref));
    colors, markers, markeredgecolors, markerfillstyles, labels : one entry per curve of ``data`` (defaults: matplotlib's property
    cycle, round full markers, ``$c_i$``); gray, black : the colors of guide lines;
    sample_method : 'svd' (default) reproduces the reference's draws on the host and needs scipy's eigendecomposition of ``cov``
    (slow at large n); 'cholesky' is the device sampler of ``Diagnostic.samples``;
    device, backend : as for ``Diagnostic`` ('hip', the default, or 'cpu'; $GSUM_BACKEND).
    ``close()`` frees the device factors.
    """

    def __init__(self, data, mean, cov, df=None, random_state=1, nref=1000, colors=None, markers=None, labels=None,
                 gray='lightgray', black='#262626', markeredgecolors=None, markerfillstyles=None, sample_method='svd',
                 device=None, backend=None):
        self.diagnostic = Diagnostic(mean=mean, cov=cov, df=df, random_state=random_state, device=device, backend=backend)
        self.device, self.backend = device, self.diagnostic.backend
        data = np.asarray(data, dtype=float)
        self.data = data[:, None] if data.ndim == 1 else data                      # always (n_samples, n_curves)
        samples = self.diagnostic.samples(nref, method=sample_method)
        self.samples = samples[:, None] if samples.ndim == 1 else samples
        self.labels = np.array([f"$c_{{{i}}}$" for i in range(self.data.shape[1])]) if labels is None else labels
        self.colors, self.markers = colors, markers
        self.markeredgecolors, self.markerfillstyles = markeredgecolors, markerfillstyles
        self.marker_cycle = self.color_cycle = None                               # cyclers, made with the style defaults
        self.gray, self.black = gray, black
        n = len(cov)                                                              # md^2 ~ chi2_n, or a scaled F under a Student t
        self.md_ref_dist = stats.chi2(df=n) if df is None else stats.f(dfn=n, dfd=df, scale=(df - 2) * n / df)

    def close(self):
        self.diagnostic.close()

    # ---- data accessors: no matplotlib ------------------------------------------------------------------------------------------

    def _error_func(self, kind):
        if kind not in _KINDS:
            raise ValueError(f"kind must be one of {_KINDS}, got {kind!r}")
        return getattr(self.diagnostic, kind + "_errors")

    def _qq_numbers(self, func, data, ref, band_perc):
        """(q_theory, sorted func(data), bands of sorted func(ref)): the one place the QQ numbers are made"""
        where = dict(device=self.device, backend=self.backend)
        q = _band_percentiles(band_perc)
        bands = refdist.qq_bands(func(np.array(ref)), q.ravel(), **where).reshape(q.shape + (-1,))
        data_sorted = refdist.sort_columns(func(np.array(data)), **where)
        n = data_sorted.shape[0]
        q_theory = self.diagnostic.std_udist.ppf((np.arange(1, n + 1) - 0.5) / n)
        return q_theory, data_sorted, bands

    def error_data(self, kind):
        """``(err, (lo, hi))``: the errors of ``data``, shape (n_samples, n_curves), and the -2 / +2 standard deviation lines of
        the standardised distribution."""
        sd = self.diagnostic.std_udist.std()
        return self._error_func(kind)(self.data), (-2 * sd, 2 * sd)

    def qq_data(self, kind, band_perc=_DEFAULT_BANDS):
        """``(q_theory, data_sorted, bands)`` of a QQ plot: the theoretical quantiles (n_samples,), the errors of ``data`` with every
        curve sorted (n_samples, n_curves), and for every b of ``band_perc`` the 100(1-b)/2 and 100(1+b)/2 percentiles over the
        reference curves of their sorted errors, shape (len(band_perc), 2, n_samples)."""
        return self._qq_numbers(self._error_func(kind), self.data, self.samples, band_perc)

    def credible_interval_data(self, intervals, band_perc):
        """``(dci_data, bands)``: the empirical coverage of every credible interval by every curve of ``data``, shape (n_curves,
        n_intervals), and the percentile bands of the same diagnostic over the reference curves, (len(band_perc), 2,
        n_intervals).  The interval bounds are taken once on the host; the coverages are ``refdist.interval_coverage``."""
        lower, upper = self.diagnostic.udist.interval(np.atleast_2d(intervals).T)
        where = dict(device=self.device, backend=self.backend)
        dci_data = refdist.interval_coverage(self.data, lower, upper, **where)
        dci_ref = refdist.interval_coverage(self.samples, lower, upper, **where)
        bands = np.array([np.percentile(dci_ref, list(p), axis=0) for p in _band_percentiles(band_perc)])
        return dci_data, bands

    def md_data(self):
        """``(md_squared(data), md_ref_dist)``: the squared Mahalanobis distance of every curve and its reference distribution."""
        return self.diagnostic.md_squared(self.data), self.md_ref_dist

    # ---- drawing helpers --------------------------------------------------------------------------------------------------------

    def _pyplot(self):
        """matplotlib.pyplot; on the first call the style lists left at None are filled from the property cycle"""
        import matplotlib
        import matplotlib.pyplot as pyplot
        if self.color_cycle is None:
            from cycler import cycler
            entries = list(matplotlib.rcParams['axes.prop_cycle'])
            defaults = dict(colors=[e['color'] for e in entries], markers=['o'] * len(entries),
                            markeredgecolors=[None] * len(entries), markerfillstyles=['full'] * len(entries))
            for name, value in defaults.items():
                if getattr(self, name) is None:
                    setattr(self, name, value)
            self.marker_cycle = cycler('marker', self.colors)
            self.color_cycle = cycler('color', self.colors)
        return pyplot

    def _axis(self, ax):
        pyplot = self._pyplot()
        return pyplot.gca() if ax is None else ax

    @staticmethod
    def _draw(ax, artists, title=None, xlabel=None, ylabel=None, force_text=False):
        """Draw a list of (kind, data, style) in order -- 'hline' y, 'vline' x, 'line' (x, y), 'band' (x, low, high), 'hist'
        values -- then set the texts that are given (all three, None included, with ``force_text``)."""
        for kind, data, style in artists:
            if kind == 'hline':
                ax.axhline(data, 0, 1, **style)
            elif kind == 'vline':
                ax.axvline(data, 0, 1, **style)
            elif kind == 'line':
                ax.plot(data[0], data[1], **style)
            elif kind == 'band':
                ax.fill_between(data[0], data[1], data[2], **style)
            elif kind == 'hist':
                ax.hist(data, density=1, histtype='step', **style)
            else:
                raise ValueError(kind)
        for setter, text in ((ax.set_title, title), (ax.set_xlabel, xlabel), (ax.set_ylabel, ylabel)):
            if force_text or text is not None:
                setter(text)
        return ax

    def _marker_style(self, i):
        return dict(ls='', color=self.colors[i], marker=self.markers[i], markeredgecolor=self.markeredgecolors[i],
                    fillstyle=self.markerfillstyles[i], markersize=8, markeredgewidth=0.5)

    # ---- panels -----------------------------------------------------------------------------------------------------------------

    def error_plot(self, err, title=None, xlabel='Index', ylabel=None, ax=None):
        """Errors against their index, one marker set per curve, over a zero line and the +-2 sd lines of the standardised
        distribution."""
        ax = self._axis(ax)
        err = np.asarray(err)
        err = err[:, None] if err.ndim == 1 else err
        two_sd = 2 * self.diagnostic.std_udist.std()
        index = np.arange(1, self.data.shape[0] + 1)
        guide = dict(zorder=0, lw=1)
        artists = [('hline', 0, dict(guide, color=self.black, linestyle='-')),
                   ('hline', -two_sd, dict(guide, color=self.gray)), ('hline', two_sd, dict(guide, color=self.gray))]
        artists += [('line', (index, column), self._marker_style(i)) for i, column in enumerate(err.T)]
        from matplotlib import ticker
        ax.xaxis.set_major_locator(ticker.MaxNLocator(integer=True))       # indices are whole numbers
        ax.margins(x=0.05)                                                  # room for the outermost markers
        return self._draw(ax, artists, title, xlabel, ylabel, force_text=True)

    def _errors_panel(self, kind, title, ax):
        return self.error_plot(self.error_data(kind)[0], title=title, ax=ax)

    def _qq_panel(self, kind, title, ax):
        return self._qq_draw(*self.qq_data(kind, _DEFAULT_BANDS), title=title, ax=ax)

    def individual_errors(self, title='Individual Errors', ax=None):
        return self._errors_panel('individual', title, ax)

    def individual_errors_qq(self, title='Individual QQ Plot', ax=None):
        return self._qq_panel('individual', title, ax)

    def cholesky_errors(self, title='Cholesky Errors', ax=None):
        return self._errors_panel('cholesky', title, ax)

    def cholesky_errors_qq(self, title='Cholesky QQ Plot', ax=None):
        return self._qq_panel('cholesky', title, ax)

    def pivoted_cholesky_errors(self, title='Pivoted Cholesky Errors', ax=None):
        return self._errors_panel('pivoted_cholesky', title, ax)

    def pivoted_cholesky_errors_qq(self, title='Pivoted Cholesky QQ Plot', ax=None):
        return self._qq_panel('pivoted_cholesky', title, ax)

    def eigen_errors(self, title='Eigen Errors', ax=None):
        return self._errors_panel('eigen', title, ax)

    def eigen_errors_qq(self, title='Eigen QQ Plot', ax=None):
        return self._qq_panel('eigen', title, ax)

    def hist(self, data, ref, title=None, xlabel=None, ylabel=None, vlines=True, ax=None):
        """``data`` against a reference that is either a frozen scipy distribution (its density between the 97.5 % and 2.5 %
        points) or a sample (a step histogram, mean +- 2 sd); the data as vertical lines, or as a histogram with
        ``vlines=False``."""
        ax = self._axis(ax)
        if hasattr(ref, 'ppf'):
            edges = (ref.ppf(0.975), ref.ppf(0.025))
            x = np.linspace(edges[0], edges[1], 100)
            artists = [('line', (x, ref.pdf(x)), dict(label='ref', color=self.black))]
        else:
            centre, spread = np.mean(ref), np.std(ref, ddof=1)
            edges = (centre - 2 * spread, centre + 2 * spread)
            artists = [('hist', ref, dict(label='ref', color=self.black))]
        dashed = dict(color='gray', linestyle='--')
        artists += [('vline', edges[0], dict(dashed, label=r'$2\sigma$')), ('vline', edges[1], dashed)]
        if vlines:
            colors = list(self.color_cycle)
            artists += [('vline', value, dict(colors[i % len(colors)], zorder=50)) for i, value in enumerate(np.atleast_1d(data))]
        else:
            artists.append(('hist', data, dict(label='data')))
        self._draw(ax, artists, title, xlabel, ylabel)
        ax.legend()
        return ax

    def violin(self, data, ref, title=None, xlabel=None, ylabel=None, ax=None):
        raise NotImplementedError("violin needs seaborn's violin and swarm plots; it is not provided")

    def box(self, data, ref, title=None, xlabel=None, ylabel=None, trim=True, size=8, legend=False, ax=None):
        raise NotImplementedError("box needs seaborn's swarm plot; it is not provided")

    def _qq_draw(self, q_theory, data_sorted, bands, title=None, ax=None):
        ax = self._axis(ax)
        shade = dict(alpha=0.5, color='gray')
        artists = [('band', (q_theory, low, high), shade) for low, high in bands[::-1]]         # last (widest) band first
        artists += [('line', (q_theory, column), dict(c=self.colors[i], label=self.labels[i])) for i, column in enumerate(data_sorted.T)]
        self._draw(ax, artists)
        xlim, ylim = ax.get_xlim(), ax.get_ylim()                                                 # the diagonal must not move them
        self._draw(ax, [('line', (xlim, xlim), dict(c=self.black))], title, 'Theoretical Quantiles', 'Empirical Quantiles')
        ax.set_xlim(xlim)
        ax.set_ylim(ylim)
        return ax

    def qq(self, data, ref, band_perc, func, title=None, ax=None):
        """The general QQ panel: ``func`` maps curves (n_samples, n_curves) to their diagnostic; the sort and the bands of
        ``func(ref)`` go through ``refdist`` on this object's backend."""
        return self._qq_draw(*self._qq_numbers(func, data, ref, band_perc), title=title, ax=ax)

    def md_squared(self, ax=None, type='hist', title='Mahalanobis Distance', xlabel='MD', **kwargs):
        if type == 'box':
            return self.box(None, None)
        if type != 'hist':
            return None
        md, ref = self.md_data()
        return self.hist(md, ref, title=title, xlabel=xlabel, ax=self._axis(ax), **kwargs)

    def kl(self, X, gp, predict=False, vlines=True, title='KL Divergence', xlabel='KL', ax=None):
        raise NotImplementedError("the KL panel is not provided: the reference refits `gp` to slices of `samples` along the points "
                                  "axis, which defines no reference distribution to port")

    def credible_interval(self, intervals, band_perc, title='Credible Interval Diagnostic',
                          xlabel='Credible Interval', ylabel='Empirical Coverage', ax=None, linestyles=None):
        """Empirical coverage against credible interval: grey bands from the reference curves (band i of ``band_perc`` as given,
        shaded and layered by the i-th smallest fraction, as the reference pairs them), the diagonal, one line per curve."""
        ax = self._axis(ax)
        import matplotlib
        greys = matplotlib.colormaps['Greys']
        dci_data, bands = self.credible_interval_data(intervals, band_perc)
        fractions = np.sort(band_perc)
        count = len(fractions)
        artists = [('band', (intervals, bands[i, 0], bands[i, 1]), dict(alpha=1., color=greys((count - i) / (count + 2.5)), zorder=-fraction))
                   for i, fraction in enumerate(fractions)]
        artists.append(('line', ([0, 1], [0, 1]), dict(c=self.black)))
        artists += [('line', (intervals, row), dict(color=self.colors[i], label=self.labels[i], ls=None if linestyles is None else linestyles[i]))
                    for i, row in enumerate(dci_data)]
        self._draw(ax, artists, title, xlabel, ylabel, force_text=True)
        ax.set(xlim=(0, 1), ylim=(0, 1))
        return ax

    def _credible_interval_default(self, ax=None):
        return self.credible_interval(np.linspace(0, 1, 101), list(_DEFAULT_BANDS), ax=ax)

    def variogram(self, X, title='Variogram', xlabel='Lag', ax=None):
        """The empirical variogram of every curve of ``data`` at inputs X (markers) between its fourth-root bands (thin lines);
        ceil(P^(1/3)) bin bounds for P pairs, from 0 to the largest |X_i|."""
        ax = self._axis(ax)
        curves = self.data.T
        pairs = len(X) * (len(X) - 1) / 2.
        bounds = np.linspace(0, np.max(np.linalg.norm(X, axis=-1)), int(np.ceil(pairs ** (1. / 3))))
        v, lags, gamma, low, high = self.diagnostic.variogram(X, curves, bounds, device=self.device, backend=self.backend)
        v.close()
        artists = []
        for i in range(curves.shape[0]):
            thin = dict(lw=0.5, c=self.colors[i])
            artists += [('line', (lags, gamma[:, i]), dict(ls='', marker='o', c=self.colors[i])),
                        ('line', (lags, low[:, i]), thin), ('line', (lags, high[:, i]), thin)]
        return self._draw(ax, artists, title, xlabel)

    # ---- figures ----------------------------------------------------------------------------------------------------------------

    def _figure(self, layout, shape, figsize, eigen, **panel_kwargs):
        """a grid of panels from a layout table; eigen panels are drawn or, with ``eigen=False``, their axes switched off"""
        if eigen and self.backend != "cpu":
            raise NotImplementedError(_EIGEN_MESSAGE)
        fig, axes = self._pyplot().subplots(*shape, figsize=figsize)
        for where, method, needs_eigen in layout:
            if needs_eigen and not eigen:
                axes[where].set_axis_off()
            else:
                getattr(self, method)(ax=axes[where], **panel_kwargs.get(method, {}))
        fig.tight_layout()
        return fig, axes

    def plotzilla(self, X, gp=None, predict=False, vlines=True, eigen=True):
        R"""Every panel in one 4 x 3 figure (the KL panel's axis stays empty).  ``eigen=False`` switches the two eigen axes off; on
        backend='hip' ``eigen=True`` raises before anything is drawn."""
        if gp is not None:
            raise NotImplementedError("plotzilla(gp=...) needs the KL panel, which is not provided")
        return self._figure(_PLOTZILLA, (4, 3), (12, 12), eigen, md_squared=dict(vlines=vlines))

    def essentials(self, vlines=True, bare=False, eigen=True):
        R"""``bare=True``: the three-panel figure (Mahalanobis distance, pivoted Cholesky errors, credible intervals) without
        titles or y labels, each panel tagged D_MD, D_PC, D_CI; it has no eigen panel and works on every backend.
        ``bare=False``: 2 x 3 panels with the eigen errors and their QQ plot: ``eigen=False`` switches those two axes off; on
        backend='hip' ``eigen=True`` raises before anything is drawn."""
        if not bare:
            return self._figure(_ESSENTIALS, (2, 3), (12, 6), eigen, md_squared=dict(vlines=vlines))
        fig, axes = self._pyplot().subplots(1, 3, figsize=(7, 3))
        for col, method, _ in _ESSENTIALS_BARE:
            getattr(self, method)(ax=axes[col], **(dict(vlines=vlines) if method == "md_squared" else {}))
        for col, _, name in _ESSENTIALS_BARE:
            ax = axes[col]
            ax.set_title('')
            ax.set_ylabel('')
            if name != "CI":
                ax.set_yticks([])
                ax.legend(title=_tag(name))
        ci = axes[2]
        ci.set_xticks([0, 0.5, 1])
        ci.set_xticklabels(['0', '0.5', '1'])
        ci.yaxis.tick_right()
        ci.text(0.05, 0.94, _tag("CI"), transform=ci.transAxes, va='top',
                bbox={'boxstyle': 'round', 'facecolor': 'white', 'alpha': 0.5, 'ec': 'grey'})
        fig.tight_layout(h_pad=0.01, w_pad=0.1)
        return fig, axes
