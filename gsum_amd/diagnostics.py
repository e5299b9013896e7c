"""Model checking (gsum/diagnostics.py:21-171; helpers.py:185-199, 504-523): ``Diagnostic`` and ``pivoted_cholesky``.

The square roots of the covariance are device factors: ``cov`` is uploaded once and factorised twice on the device, once as
numpy.linalg.cholesky (potrf) and once as LAPACK dpstrf (the pivoted Cholesky of this library); both stay
resident until ``close()``.  Errors and Mahalanobis distances of any number of curves are one ``gsum_sqrt_errors`` call each.
What is O(n x curves) on the host in the reference stays on the host here (individual errors, chi2, credible intervals, the
default samples), with the reference's own arithmetic.

``Diagnostic.variogram`` is ``VariogramFourthRoot`` (variogram.py, libgsum_vario.so) followed by its ``compute()``.

``GraphicalDiagnostic`` (graphical.py) owns a ``Diagnostic`` and puts its results beside reference distributions made by simulation;
the band stage of those runs in libgsum_refdist.so (refdist.py).

``TruncationPointwise`` is pointwise.py.  Not provided: a device eigensolver (``eigen_errors`` runs on ``backend='cpu'`` only, and with it the
eigen panels of ``GraphicalDiagnostic``).
"""
from __future__ import annotations


import numpy as np
import scipy.stats as stats

from ._backend import resolve_backend
from ._lib import ChainAborted, default_context

__all__ = ["Diagnostic", "pivoted_cholesky"]


def _context(device, backend):
    backend = resolve_backend(backend)
    if backend == "cpu":
        from ._cpu import cpu_context
        return cpu_context(), backend
    return default_context(device), backend


def _factor(ctx, A, pivot):
    """Upload A and factorise it (pivot: dpstrf) -> the resident factor; LinAlgError where A is not positive definite."""
    for attempt in (0, 1):
        M = ctx.upload(A)
        try:
            info = ctx.pstrf(M)[0] if pivot else ctx.potrf(M)
        except ChainAborted:                   # the single-factorisation schedule gave up: the library has switched it off, once more
            M.free()
            if attempt:
                raise
            continue
        except BaseException:
            M.free()
            raise
        if info:
            M.free()
            raise np.linalg.LinAlgError("Matrix is not positive definite" if not pivot else "M is not positive-semidefinite")
        return M


def pivoted_cholesky(M, device=None, backend=None):
    """G with M = G G^T: the dpstrf factor with its rows put back in M's order (helpers.py:185-199).  LinAlgError when M is
    rank-deficient."""
    M = np.asarray(M, dtype=float)
    ctx, _ = _context(device, backend)
    F = _factor(ctx, M, pivot=True)
    try:
        L = F.to_host()
        p = np.asarray(F.piv)
    finally:
        F.free()
    p_inv = np.arange(len(p))[np.argsort(p)]
    return L[p_inv]


class Diagnostic:
    R"""Bastos & O'Hagan's model checks for N(mean, cov) (or a multivariate t with ``df``): gsum.diagnostics.Diagnostic.

    ``device`` / ``backend`` ('hip', the default, or 'cpu'; $GSUM_BACKEND) as for the model classes.  A covariance that is not
    positive definite raises numpy.linalg.LinAlgError.  Call ``close()`` to free the two device factors (``__del__`` does too).
    """

    def __init__(self, mean, cov, df=None, random_state=1, device=None, backend=None):
        self.mean = mean
        self.cov = cov
        self.df = df
        self.random_state = random_state
        self.sd = sd = np.sqrt(np.diag(cov))
        if df is None:
            self.udist = stats.norm(loc=mean, scale=sd)
            self.std_udist = stats.norm(loc=0., scale=1.)
        else:
            self.udist = stats.t(loc=mean, scale=sd, df=df)
            self.std_udist = stats.t(loc=0., scale=1., df=df)
        self.udist.random_state = random_state
        self.std_udist.random_state = random_state
        self._dist = None
        self._rng = np.random.RandomState(random_state)
        self._eig = None
        self._ctx, self.backend = _context(device, backend)
        cov = np.asarray(cov, dtype=float)
        self._mean = np.ascontiguousarray(np.broadcast_to(np.asarray(mean, dtype=float), (cov.shape[0],)))
        self._L = self._P = self._loo = None
        self._L = _factor(self._ctx, cov, pivot=False)
        self._P = _factor(self._ctx, cov, pivot=True)

    def close(self):
        if getattr(self, "_loo", None) is not None:
            self._loo.free()
            self._loo = None
        for name in ("_L", "_P"):
            M = getattr(self, name, None)
            if M is not None:
                M.free()
                setattr(self, name, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _errors(self, y, pivot, errors=True, md2=False):
        if self._L is None:
            raise ValueError("Diagnostic is closed")
        return self._ctx.sqrt_errors(self._P if pivot else self._L, np.asarray(y, dtype=float), self._mean, pivot=pivot, errors=errors,
                                     md2=md2)

    def samples(self, n, method="svd"):
        R"""n curves, shape (n_samples, n_curves).  ``method='svd'`` (default): the reference's draws -- scipy's frozen
        multivariate_normal with ``random_state`` -- on the host.  ``'cholesky'``: mean + L z on the device.  With ``df`` the draws
        are the multivariate t of statsmodels' MVT (mean + N(0, sigma) / sqrt(chi2_df / df), sigma = cov (df - 2) / df) on the device:
        the same distribution, not the same numbers."""
        if method not in ("svd", "cholesky"):
            raise ValueError("method must be 'svd' or 'cholesky'")
        if method == "svd" and self.df is None:
            if self._dist is None:
                self._dist = stats.multivariate_normal(mean=self.mean, cov=self.cov)
                self._dist.random_state = self.random_state
            return self._dist.rvs(n).T
        dim = self._mean.shape[0]
        z = self._rng.standard_normal((dim, n))
        out = self._ctx.tri_multiply(self._L, z)
        if self.df is not None:
            w = self._rng.chisquare(self.df, n) / self.df
            out = out * np.sqrt((self.df - 2) / self.df) / np.sqrt(w)[None, :]
        out = out + self._mean[:, None]
        return out[:, 0] if n == 1 else out

    def individual_errors(self, y):
        R"""D_I(y) = (y - m) / sigma, shape (n_samples, [n_curves])."""
        return ((np.asarray(y, dtype=float).T - self.mean) / self.sd).T

    def cholesky_errors(self, y):
        return self._errors(y, pivot=False)[0]

    def pivoted_cholesky_errors(self, y):
        return self._errors(y, pivot=True)[0]

    def eigen_errors(self, y):
        if self.backend != "cpu":
            raise NotImplementedError("eigen_errors needs a symmetric eigensolver, which the device library does not provide; "
                                      "use backend='cpu'")
        if self._eig is None:                                                   # eigenvalues largest first (Bastos & O'Hagan)
            w, V = np.linalg.eigh(self.cov)
            self._eig = V[:, ::-1] @ np.diag(np.sqrt(w[::-1]))
        return np.linalg.solve(self._eig, (np.asarray(y, dtype=float).T - self.mean).T)

    def loo(self, y):
        R"""The leave-one-out predictions of y, (n_samples, [n_curves]): each point against all the others (``LooResult``; loo.py).
        The resident factor goes to the host and into the leave-one-out library once; its inverse stays there until ``close()``."""
        if self.df is not None:
            raise NotImplementedError("loo is the Gaussian leave-one-out; a Student-t leave-one-out (df set) is not provided")
        return self._loo_factor().loo(y, self._mean)

    def _loo_factor(self):
        if self._L is None:
            raise ValueError("Diagnostic is closed")
        if self._loo is None:
            from .loo import LooFactor
            self._loo = LooFactor(self._L.to_host(), device=self._ctx.device, backend=self.backend)
        return self._loo

    def kfold(self, y, folds):
        R"""The leave-group-out predictions of y, (n_samples, [n_curves]): every point against the points outside its group
        (``FoldResult``; ``folds`` as in ``LooFactor.folds``).  It shares the resident inverse factor with ``loo``."""
        if self.df is not None:
            raise NotImplementedError("kfold is the Gaussian leave-group-out; a Student-t one (df set) is not provided")
        return self._loo_factor().folds(y, folds, self._mean)

    def loo_errors(self, y):
        R"""The standardised leave-one-out errors a_i / sqrt(p_i), shape (n_samples, [n_curves])."""
        return self.loo(y).error

    def chi2(self, y):
        return np.sum(self.individual_errors(y), axis=0)

    def md_squared(self, y):
        R"""The squared Mahalanobis distance, one per curve."""
        return self._errors(y, pivot=False, errors=False, md2=True)[1]

    def kl(self, mean, cov):
        R"""KL divergence D(N_0 | N_1) with N_1 this object's distribution and N_0 = N(mean, cov): tr(Sigma_1^-1 Sigma_0) is the
        summed md2 of the columns of chol(Sigma_0) against the resident factor; the log term keeps the reference's
        2 sum log diag(Sigma_1) (diagnostics.py:145: the covariance's diagonal, not its factor's)."""
        c0 = np.asarray(cov, dtype=float)
        F = _factor(self._ctx, c0, pivot=False)
        try:
            L0 = F.to_host()
        finally:
            F.free()
        tr = float(np.sum(self._ctx.sqrt_errors(self._L, L0, None, pivot=False, errors=False, md2=True)[1]))
        dist = self.md_squared(mean)
        k = np.asarray(self.cov).shape[-1]
        logs = 2 * np.sum(np.log(np.diag(self.cov))) - 2 * np.sum(np.log(np.diag(L0)))
        return 0.5 * (tr + dist - k + logs)

    @staticmethod
    def variogram(X, y, bin_bounds, device=None, backend=None):
        R"""The variogram of the curves y (shape (N,) or (n_curves, N)) at inputs X: (v, bin_locations, gamma, lower, upper), v the
        VariogramFourthRoot and the rest its ``compute(rt_scale=False)`` (diagnostics.py:173-194)."""
        from .variogram import VariogramFourthRoot
        v = VariogramFourthRoot(X, y, bin_bounds, device=device, backend=backend)
        bin_locations = v.bin_locations
        gamma, lower, upper = v.compute(rt_scale=False)
        return v, bin_locations, gamma, lower, upper

    def credible_interval(self, y, intervals):
        """The credible interval diagnostic, shape ([n_curves], n_intervals) (diagnostics.py:148-171)."""
        lower, upper = self.udist.interval(np.atleast_2d(intervals).T)          # (n_intervals, n_samples) each
        rows = np.atleast_2d(y).T                                               # one row per curve (1-D y: one per sample)
        out = np.stack([np.average((lower < r) & (r < upper), axis=1) for r in rows])
        return np.squeeze(out) if np.ndim(y) == 1 else out
