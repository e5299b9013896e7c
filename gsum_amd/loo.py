"""Leave-one-out diagnostics of N(mean, K) from one Cholesky factor K = L L^T (Rasmussen & Williams 5.4.2).

With r = y - mean, a = K^-1 r and p = diag(K^-1), the prediction of point i from all the others is closed-form:

    loo_mean_i   = y_i - a_i / p_i
    loo_var_i    = 1 / p_i
    loo_error_i  = a_i / sqrt(p_i)                               (standardised: N(0, 1) under the model)
    loo_logpdf_i = -1/2 log 2 pi + 1/2 log p_i - 1/2 a_i^2 / p_i

p needs W = L^-1 (p_j = sum_i W_ij^2), the only O(n^3) piece.  On ``backend='hip'`` libgsum_loo.so (include/gsum_loo.h, DESIGN.md
section 15) forms W on the device and keeps it there; ``backend='cpu'`` is the same arithmetic on scipy's ``solve_triangular``.
``Diagnostic.loo`` and ``ConjugateGaussianProcess.loo`` are built on ``LooFactor``.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from ._backend import resolve_backend, resolve_device

__all__ = ["LooResult", "LooFactor", "loo_from_factor"]

LooResult = namedtuple("LooResult", ["mean", "var", "error", "logpdf", "precision_diag"])
LooResult.__doc__ = """The leave-one-out predictions of every point: ``mean``, ``error`` and ``logpdf`` have y's shape, (n,) or
(n, n_curves); ``var`` and ``precision_diag`` (p = diag(K^-1) = 1 / var) are (n,), the same for every curve."""


class _CpuLoo:
    """The host stand-in for ``_loo_lib.DeviceLoo``."""

    def __init__(self, L):
        from scipy.linalg import solve_triangular
        d = np.diag(L)
        bad = np.flatnonzero(~(np.isfinite(d) & (d > 0)))
        if bad.size:
            raise ValueError(f"the factor's diagonal entry {bad[0]} is not a finite positive number")
        self.n = L.shape[0]
        self._W = solve_triangular(np.tril(L), np.eye(self.n), lower=True)          # the upper triangle is ignored, as on the device
        self._sld = float(np.sum(np.log(d)))

    def precision_diag(self):
        return (self._W * self._W).sum(0), self._sld

    def solve(self, R):
        return self._W.T @ (self._W @ R)

    def free(self):
        self._W = None


class LooFactor:
    """W = L^-1 of a lower Cholesky factor L (n x n; the upper triangle is ignored), kept for any number of ``loo`` calls: on the
    device (``backend='hip'``, the default) until ``free()``, or on the host (``'cpu'``).  ValueError where L is not square or its
    diagonal is not finite and positive."""

    def __init__(self, L, device=None, backend=None):
        self.backend = resolve_backend(backend)
        L = np.asarray(L, dtype=float)
        if L.ndim != 2 or L.shape[0] != L.shape[1] or L.shape[0] < 1:
            raise ValueError(f"L must be square and non-empty, got shape {L.shape}")
        self.n = L.shape[0]
        if self.backend == "cpu":
            self._f = _CpuLoo(L)
        else:
            from ._loo_lib import DeviceLoo
            self._f = DeviceLoo(resolve_device(device), L)
        self.precision_diag, self.sum_log_diag = self._f.precision_diag()

    def solve(self, R):
        """(L L^T)^-1 R, R of shape (n, k)."""
        return self._f.solve(np.ascontiguousarray(R, dtype=float))

    def loo(self, y, mean=0.0):
        """``LooResult`` of the curves y, (n,) or (n, n_curves), under N(mean, L L^T); ``mean`` a scalar or (n,)."""
        y = np.asarray(y, dtype=float)
        if y.ndim not in (1, 2) or y.shape[0] != self.n or y.size == 0:
            raise ValueError(f"y must be ({self.n},) or ({self.n}, n_curves), got {y.shape}")
        mean = np.asarray(mean, dtype=float)
        if mean.shape not in ((), (self.n,)):
            raise ValueError(f"mean must be a scalar or ({self.n},), got {mean.shape}")
        r = (y.T - mean).T
        a = self.solve(r.reshape(self.n, -1)).reshape(y.shape)
        p = self.precision_diag
        pc = p if y.ndim == 1 else p[:, None]
        return LooResult(mean=y - a / pc, var=1.0 / p, error=a / np.sqrt(pc),
                         logpdf=-0.5 * np.log(2 * np.pi) + 0.5 * np.log(pc) - 0.5 * a * a / pc, precision_diag=p)

    def times(self, reset=False):
        """Device milliseconds by phase (``_loo_lib.PHASES``); 'hip' only."""
        return self._f.times(reset)

    def free(self):
        if self._f is not None:
            self._f.free()
            self._f = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def loo_from_factor(L, y, mean=0.0, device=None, backend=None):
    """``LooResult`` of y, (n,) or (n, n_curves), under N(mean, L L^T) from the lower Cholesky factor L alone."""
    f = LooFactor(L, device=device, backend=backend)
    try:
        return f.loo(y, mean)
    finally:
        f.free()
