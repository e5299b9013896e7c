"""Reference distributions by simulation: what gsum's GraphicalDiagnostic does to the diagnostics of its ``nref`` sampled curves
(gsum/diagnostics.py, ``qq`` and ``credible_interval``): sort along the points, percentile bands across the curves, credible
interval coverages.

``backend='hip'`` (the default; $GSUM_BACKEND) runs in libgsum_refdist.so (include/gsum_refdist.h): the
matrix is uploaded once, transposed, sorted in LDS and picked from on the device.  ``backend='cpu'`` evaluates the numpy expression
given with each function.  Explicit, never a silent fallback: without the library or a GPU the 'hip' backend raises.

    sort_columns(A)                    np.sort(A, axis=0)
    row_percentiles(A, q)              np.percentile(A, q, axis=1)
    qq_bands(E, q)                     np.percentile(np.sort(E, axis=0), q, axis=1)
    interval_coverage(Y, lower, upper) [mean_i(lower[k, i] < Y[i, j] < upper[k, i])]_{j, k}
"""
from __future__ import annotations

import numpy as np

from ._backend import resolve_backend, resolve_device

__all__ = ["sort_columns", "row_percentiles", "qq_bands", "interval_coverage", "device_matrix"]


def _matrix(a, name):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{name} must be 2-D and non-empty, got shape {a.shape}")
    return a


def _percents(q):
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or q.shape[0] < 1 or not np.all((q >= 0) & (q <= 100)):
        raise ValueError("percentiles must be a non-empty 1-D sequence in [0, 100]")
    return q


def device_matrix(A, device=None):
    """A (n, m) uploaded to the device: the ``DeviceRefDist`` of _refdist_lib (``sort_columns``, ``row_percentiles``, ``qq_bands``,
    ``coverage``, ``times``, ``free``), for several operations on one upload."""
    from ._refdist_lib import DeviceRefDist
    return DeviceRefDist(resolve_device(device), _matrix(A, "A"))


def sort_columns(A, device=None, backend=None):
    """Every column ascending: ``np.sort(A, axis=0)``, NaN last.  Bit-equal to numpy's for finite and infinite values (-0.0 and
    +0.0 compare equal and may come in either order; a NaN comes back positive)."""
    A = _matrix(A, "A")
    backend = resolve_backend(backend)
    if backend == "cpu":
        return np.sort(A, axis=0)
    with device_matrix(A, device) as M:
        return M.sort_columns()


def row_percentiles(A, q, device=None, backend=None):
    """``np.percentile(A, q, axis=1)`` (the default 'linear' method), shape (len(q), n); a row with a NaN gives NaN."""
    A = _matrix(A, "A")
    q = _percents(q)
    backend = resolve_backend(backend)
    if backend == "cpu":
        return np.percentile(A, q, axis=1)
    with device_matrix(A, device) as M:
        return M.row_percentiles(q)


def qq_bands(E, q, return_sorted=False, device=None, backend=None):
    """The bands of a QQ plot of the errors E (n points x m curves): ``np.percentile(np.sort(E, axis=0), q, axis=1)``, shape
    (len(q), n).  ``return_sorted=True`` returns ``(bands, np.sort(E, axis=0))``; without it the sorted matrix stays on the
    device."""
    E = _matrix(E, "E")
    q = _percents(q)
    backend = resolve_backend(backend)
    if backend == "cpu":
        S = np.sort(E, axis=0)
        bands = np.percentile(S, q, axis=1)
    else:
        with device_matrix(E, device) as M:
            bands, S = M.qq_bands(q, return_sorted=return_sorted)
    return (bands, S) if return_sorted else bands


def interval_coverage(Y, lower, upper, device=None, backend=None):
    """The credible-interval diagnostic of the curves Y (n points x m curves) for K intervals (lower, upper: K x n): shape (m, K),
    entry [j, k] the fraction of points i with ``lower[k, i] < Y[i, j] < upper[k, i]`` (both strict, false for NaN), computed as
    integer counts / n.  The intervals need not be nested or sorted."""
    Y = _matrix(Y, "Y")
    lower = _matrix(lower, "lower")
    upper = _matrix(upper, "upper")
    n = Y.shape[0]
    if lower.shape != upper.shape or lower.shape[1] != n:
        raise ValueError(f"lower and upper must both be (K, {n}), got {lower.shape} and {upper.shape}")
    backend = resolve_backend(backend)
    if backend == "cpu":
        return np.stack([np.average((lower < r) & (r < upper), axis=1) for r in Y.T])
    with device_matrix(Y, device) as M:
        return M.coverage(lower, upper) / n
