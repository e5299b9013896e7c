"""``TruncationPointwise`` (gsum/models.py:1573-1836): the uncorrelated, point-by-point truncation model.

Every point of the input space carries its own Student-t truncation error, from a scaled inverse chi squared prior on the variance
of its coefficients.  ``fit`` and the thin calls on ``scipy.stats.t`` (``interval``, ``pdf``, ``logpdf``, ``std``) are O(n * orders)
and stay on the host on every backend, so the fitted numbers equal the reference's bit for bit.  The two heavy methods run in
libgsum_pointwise.so (include/gsum_pointwise.h) on ``backend='hip'``:

* ``log_likelihood`` / ``log_likelihood_grid``: the likelihood of a whole grid of candidate ratios (the breakdown-scale posterior
  of the reference's ``truncation_recap`` notebook) in one device call;
* ``credible_diagnostic``: the success rates are counted on the device without ever forming the (len(dobs), n, n_orders) bounds.

``backend='cpu'`` evaluates the reference's numpy / scipy expressions.  Explicit, never a silent fallback: without the library or a
GPU the 'hip' backend raises.
"""
from __future__ import annotations

import numpy as np
import scipy.stats as st
from scipy.special import loggamma

from ._backend import resolve_backend, resolve_device
from .series import coefficients, geometric_sum
from .stats import hpd

__all__ = ["TruncationPointwise"]


class TruncationPointwise:
    R"""The pointwise convergence model of Furnstahl et al. (2015) by conjugacy: gsum.models.TruncationPointwise.

    ``y_k = y_ref sum_{n<=k} c_n Q^n`` with iid ``c_n | cbar^2 ~ N(0, cbar^2)`` and ``cbar^2 ~ chi^-2(df, scale^2)``.

    df : float >= 0, scale : float > 0 -- the prior's degrees of freedom and scale; excluded : int or array, optional -- orders left
    out of the update and of the truncation error; backend : 'hip' (the default; $GSUM_BACKEND) or 'cpu'; device : the GPU index
    ($GSUM_DEVICE).  ``close()`` frees the device copy of the data.

    Fitted attributes, as in the reference: ``y_``, ``ratio_``, ``ref_``, ``orders_``, ``orders_mask_``, ``coeffs_``, ``df_``,
    ``scale_``, ``y_masked_``, ``coeffs_dist_``, ``dist_``.

    The reference's behaviour is kept where it surprises:

    * ``log_likelihood`` adds ``loggamma(df / 2) - n_orders / 2 * log(2 pi)`` and, for ``df0 > 0``, the prior's term ONCE, not once per
      point (models.py:1792-1794);
    * ``df0 == 0`` drops the prior's term altogether (models.py:1793);
    * the change-of-variables term ``log|ref| + sum(orders) * log(ratio)`` is summed over whatever ``ref`` and ``ratio`` broadcast
      to (models.py:1796): a scalar ``ratio`` with a scalar ``ref`` (a length-1 array counts as a scalar) counts it once, and as
      soon as either is an ``(n,)`` array it is counted n times;
    * ``interval``, ``pdf`` and ``logpdf`` select ``orders`` through an index that is squeezed (models.py:1644): one order drops the
      orders axis, several keep it.

    On 'hip' the orders must be integers, between 1 and 64 of them kept, and ``ratio ** order`` is taken by repeated multiplication.
    """

    def __init__(self, df=1, scale=1, excluded=None, backend=None, device=None):
        self.df0 = df
        self.scale0 = scale
        self.excluded = excluded
        self.backend = resolve_backend(backend)
        self.device = device
        self._fit = False
        self._dev = None
        self.y_ = self.ratio_ = self.ref_ = self.orders_ = self.orders_mask_ = self._orders_masked = None
        self.coeffs_ = self.coeffs_dist_ = self.df_ = self.scale_ = self.y_masked_ = self.dist_ = None
        self._trunc_scale = None

    # ---- the conjugate update -----------------------------------------------------------------------------------------------------

    @classmethod
    def _compute_df(cls, c, df0):
        return df0 + c.shape[-1]

    @classmethod
    def _compute_scale(cls, c, df0, scale0):
        return np.sqrt((df0 * scale0 ** 2 + (c ** 2).sum(-1)) / cls._compute_df(c, df0))

    def _compute_order_indices(self, orders):
        """The positions of ``orders`` among the kept orders, squeezed; everything for None."""
        if orders is None:
            return slice(None)
        return np.squeeze(np.array([np.nonzero(self._orders_masked == o)[0] for o in np.atleast_1d(orders)]))

    def fit(self, y, ratio, ref=1, orders=None):
        """Update the hyperparameters from the partial sums ``y`` (n_points, n_orders) computed at ``orders`` (default 0, 1, ...)
        with expansion parameter ``ratio`` and scale ``ref`` (scalars or (n_points,) arrays).  Host arithmetic on every backend."""
        y = np.asarray(y)
        if y.ndim == 1:
            y = y[:, None]
        ratio, ref = np.atleast_1d(ratio, ref)
        orders = np.arange(y.shape[-1]) if orders is None else np.asarray(orders)
        if y.shape[-1] != orders.size:
            raise ValueError("The last dimension of `y` must have the same size as `orders`")
        self.close()
        self.y_, self.ratio_, self.ref_, self.orders_ = y, ratio, ref, orders
        self.orders_mask_ = mask = ~np.isin(orders, self.excluded)
        self.coeffs_ = coefficients(y=y, ratio=ratio, ref=ref, orders=orders)[:, mask]
        self.df_ = self._compute_df(self.coeffs_, self.df0)
        self.scale_ = self._compute_scale(self.coeffs_, self.df0, self.scale0)
        self.y_masked_ = y[:, mask]
        self._orders_masked = orders[mask]
        tails = np.array([geometric_sum(ratio ** 2, k + 1, np.inf, excluded=self.excluded) for k in self._orders_masked]).T
        self._trunc_scale = ref[:, None] * np.sqrt(tails) * self.scale_[:, None]
        self.coeffs_dist_ = st.t(loc=0, scale=self.scale_, df=self.df_)
        self.dist_ = st.t(loc=self.y_masked_, scale=self._trunc_scale, df=self.df_)
        self._fit = True
        return self

    def close(self):
        """Free the device copy of the fitted data (made by the first 'hip' call after ``fit``)."""
        if self._dev is not None:
            self._dev.free()
            self._dev = None

    def device_times(self, reset=False):
        """Device milliseconds (HIP events) the 'hip' calls since ``fit`` have spent, by phase: h2d, differences, loglike, coverage,
        d2h."""
        return self._device_data().times(reset)

    # ---- thin calls on the truncation error distribution (host) -------------------------------------------------------------------

    @staticmethod
    def _over_points(a):
        a = np.atleast_1d(a)
        return a[:, None, None] if a.ndim == 1 else a

    def interval(self, alpha, orders=None):
        """``dist_.interval(alpha)`` as an array (2, [len(alpha)], n_points, n_orders), at ``orders`` when given."""
        alpha = np.array(alpha)
        if alpha.ndim == 1:
            alpha = alpha[:, None, None]
        return np.array(self.dist_.interval(alpha))[..., self._compute_order_indices(orders)]

    def pdf(self, y, orders=None):
        """``dist_.pdf(y)`` at ``orders``; a 1-D ``y`` runs along a new leading axis."""
        return self.dist_.pdf(self._over_points(y))[..., self._compute_order_indices(orders)]

    def logpdf(self, y, orders=None):
        """``dist_.logpdf(y)`` at ``orders``; a 1-D ``y`` runs along a new leading axis."""
        return self.dist_.logpdf(self._over_points(y))[..., self._compute_order_indices(orders)]

    def std(self):
        """``dist_.std()``: (n_points, n_orders)."""
        return self.dist_.std()

    # ---- the likelihood of ratio and ref --------------------------------------------------------------------------------------------

    def _require_fit(self, method):
        if not self._fit:
            raise ValueError(f"Must call fit before calling {method}")

    def _constants(self):
        """The terms of the log likelihood that depend on neither ratio nor ref, added once (models.py:1792-1794)."""
        df0, scale0 = self.df0, self.scale0
        kept = int(np.count_nonzero(self.orders_mask_))
        const = loggamma((df0 + kept) / 2.) - 0.5 * kept * np.log(2 * np.pi)
        if df0 > 0:
            const += 0.5 * np.sum(df0 * np.log(df0 * scale0 ** 2 / 2.)) - loggamma(df0 / 2.)
        return const

    def _log_likelihood_host(self, ratio, ref):
        orders, mask = self.orders_, self.orders_mask_
        c = coefficients(y=self.y_, ratio=ratio, ref=ref, orders=orders)[:, mask]
        df = self._compute_df(c, self.df0)
        scale = self._compute_scale(c, self.df0, self.scale0)
        log_like = self._constants()
        log_like -= 0.5 * np.sum(df * np.log(df * scale ** 2 / 2.))
        log_like -= np.sum(np.log(np.abs(ref)) + np.sum(orders[mask]) * np.log(ratio))
        return log_like

    def _device_data(self):
        if self._dev is None:
            from ._pointwise_lib import DevicePointwise
            orders = np.asarray(self.orders_)
            if not np.all(orders == np.round(orders)):
                raise ValueError("backend='hip' takes integer orders")
            self._dev = DevicePointwise(resolve_device(self.device), self.y_, orders, self.orders_mask_)
        return self._dev

    def _shared(self, a, name):
        """A ratio or ref shared by every row of a grid, as (values, per_point): a scalar or length-1 array is a scalar."""
        a = np.asarray(a, dtype=np.float64)
        n = self.y_.shape[0]
        if a.size == 1 and a.ndim <= 1:
            return a.reshape(1), False
        if a.shape == (n,):
            return a, True
        raise ValueError(f"{name} must be a scalar or an array of shape ({n},), got shape {a.shape}")

    def log_likelihood(self, ratio=None, ref=None):
        """The log likelihood of ``ratio`` and ``ref`` (each a scalar or an (n_points,) array; default: the fitted ones) given the
        data passed to ``fit``.  On 'hip' this is ``log_likelihood_grid`` with one row."""
        self._require_fit("log_likelihood")
        ratio = self.ratio_ if ratio is None else ratio
        ref = self.ref_ if ref is None else ref
        if self.backend == "cpu":
            return self._log_likelihood_host(ratio, ref)
        from ._pointwise_lib import REF_POINTS, REF_SCALAR
        ratio, _ = self._shared(ratio, "ratio")
        ref, ref_points = self._shared(ref, "ref")
        out = self._device_data().loglike_grid(ratio[None] if ratio.shape[0] > 1 else ratio, ref, REF_POINTS if ref_points else REF_SCALAR,
                                               self.df0, self.scale0)
        return self._constants() - out[0]

    def log_likelihood_grid(self, ratios, refs=None):
        """``[log_likelihood(ratio=ratios[g], ref=refs[g]) for g in range(G)]`` as a (G,) float64 array, one device call on 'hip'.

        ratios : (G,) -- one scalar ratio per row -- or (G, n_points); refs : None (the fitted ``ref_`` for every row), (G,) or
        (G, n_points).  Since row g is by definition that call, a row of scalars counts the change-of-variables term once."""
        self._require_fit("log_likelihood_grid")
        n = self.y_.shape[0]
        ratios = np.asarray(ratios, dtype=np.float64)
        G = ratios.shape[0] if ratios.ndim else 0
        if G < 1 or ratios.shape not in ((G,), (G, n)):
            raise ValueError(f"ratios must have shape (G,) or (G, {n}) with G >= 1, got {ratios.shape}")
        if refs is not None:
            refs = np.asarray(refs, dtype=np.float64)
            if refs.shape not in ((G,), (G, n)):
                raise ValueError(f"refs must be None or have shape ({G},) or ({G}, {n}), got {refs.shape}")
        if self.backend == "cpu":
            return np.array([self._log_likelihood_host(ratios[g], self.ref_ if refs is None else refs[g]) for g in range(G)], dtype=np.float64)
        from ._pointwise_lib import REF_POINTS, REF_ROW_POINTS, REF_ROW_SCALAR, REF_SCALAR
        if refs is None:
            refs, per_point = self._shared(self.ref_, "ref")
            mode = REF_POINTS if per_point else REF_SCALAR
        else:
            mode = REF_ROW_POINTS if refs.ndim == 2 else REF_ROW_SCALAR
        return self._constants() - self._device_data().loglike_grid(ratios, refs, mode, self.df0, self.scale0)

    # ---- the credible-interval diagnostic -----------------------------------------------------------------------------------------

    def _coverage_counts(self, data, dobs):
        """(len(dobs), n_orders) int64: the points whose ``data`` lie strictly inside the ``dobs`` credible intervals of ``dist_``.
        ``df_`` is one number, so the interval of point i and order j is ``t * scale_ij + loc_ij`` with the two Student-t quantiles
        ``t`` of the degree of belief alone."""
        unit = st.t(self.df_)
        t_lo, t_hi = unit.ppf((1.0 - dobs) / 2), unit.ppf((1.0 + dobs) / 2)
        loc, scale = np.broadcast_arrays(self.y_masked_, self._trunc_scale)
        if self.backend == "cpu":
            return np.stack([np.sum((lo * scale + loc < data) & (data < hi * scale + loc), axis=0) for lo, hi in zip(t_lo, t_hi)]).astype(np.int64)
        return self._device_data().coverage(loc, scale, data, t_lo, t_hi)

    def credible_diagnostic(self, data, dobs, band_intervals=None, band_dobs=None, beta=True):
        """``D_CI`` (len(dobs), n_orders): the fraction of the points whose ``data`` ((n_points,) or (n_points, n_orders)) fall
        strictly inside the ``dobs`` credible intervals of the truncation error.  With ``band_intervals`` also ``bands``
        (len(band_intervals), 2, len(band_dobs)), the range a consistent model's success rate takes with those probabilities:
        highest-density intervals of beta distributions (``beta=True``) or central binomial intervals; host scipy on every backend."""
        self._require_fit("credible_diagnostic")
        dobs = np.atleast_1d(dobs)
        data = np.asarray(data)
        if data.ndim == 1:
            data = data[:, None]
        N = self.y_.shape[0]
        D_CI = self._coverage_counts(data, dobs) / N
        if band_intervals is None:
            return D_CI
        band_dobs = dobs if band_dobs is None else np.atleast_1d(band_dobs)
        if beta:
            bands = np.array([np.array([hpd(st.beta, p, N * s + 1, N - N * s + 1) for s in band_dobs]).T
                              for p in np.atleast_1d(band_intervals)])
        else:
            edges = st.binom(n=N, p=band_dobs).interval(np.atleast_2d(band_intervals).T)
            bands = np.transpose(np.asarray(edges) / N, [1, 0, 2])
        return D_CI, bands
