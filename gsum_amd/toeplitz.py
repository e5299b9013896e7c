"""The Toeplitz likelihood path: stationary kernels on uniform one-dimensional grids.

With a stationary kernel on a uniform grid, ``R = kernel(X) + nugget I`` is symmetric Toeplitz and fixed by its first column ``t``.  The
Schur (Bareiss) recursion yields the columns of its Cholesky factor one after the other in O(n) each, and a forward substitution runs
beside it: ``G = Z^T T^-1 Z`` and ``sum_j log L_jj`` -- all a likelihood of this package is computed from -- cost O(n^2 c) instead of
O(n^3), and nothing of size n x n is stored.  The generator of the recursion is carried in extended precision (double-double on the
device, ``numpy.longdouble`` on ``backend='cpu'``); a plain fp64 recursion loses several digits on the ill-conditioned matrices the
smooth kernels give.

The result is the likelihood of the exactly Toeplitz matrix of ``t``.  ``kernel(X)`` itself is Toeplitz only up to the last bits of its
entries; on an ill-conditioned matrix that defect, times the condition number, is how far the dense path may sit from this one.
"""
from __future__ import annotations

import numpy as np

from ._backend import resolve_backend, resolve_device
from ._lib import FAMILY, GSUM_MAX_RHS, KernelDesc
from .kernels import describe_kernel

__all__ = ["uniform_grid_step", "toeplitz_column", "toeplitz_gram", "toeplitz_max_n"]


def uniform_grid_step(X, tol=4.0):
    """The step of the uniform grid X, shape (n,) or (n, 1), strictly monotone: ``max |X_i - (X_0 + i step)| <= tol eps max|X|`` with
    ``step = (X_{n-1} - X_0) / (n - 1)``.  ValueError, naming the first offending index, otherwise.  One point is a grid of step 0."""
    X = np.asarray(X, dtype=float)
    if X.ndim == 2 and X.shape[1] == 1:
        X = X[:, 0]
    elif X.ndim == 2:
        raise ValueError(f"a uniform grid has one feature, X has {X.shape[1]}")
    if X.ndim != 1 or X.size < 1:
        raise ValueError(f"X must have shape (n,) or (n, 1) with n >= 1, got {np.shape(X)}")
    if not np.all(np.isfinite(X)):
        raise ValueError(f"X is not finite at index {int(np.argmin(np.isfinite(X)))}")
    n = X.size
    if n == 1:
        return 0.0
    step = (X[-1] - X[0]) / (n - 1)
    d = np.diff(X)
    mono = d > 0 if step > 0 else d < 0
    if step == 0 or not np.all(mono):
        raise ValueError(f"X is not strictly monotone at index {int(np.argmin(mono)) + 1 if step != 0 else 1}")
    off = np.abs(X - (X[0] + np.arange(n) * step)) > tol * np.finfo(float).eps * np.max(np.abs(X))
    if np.any(off):
        raise ValueError(f"X is not a uniform grid: index {int(np.argmax(off))} is off X[0] + i * step by more than {tol} eps max|X|")
    return float(step)


def _is_stationary(desc):
    if desc.is_tree:
        return all(desc.leaf[i].family != FAMILY["dot"] for i in range(desc.n_leaves))
    return desc.family != FAMILY["dot"]


def _context(device, backend):
    if resolve_backend(backend) == "cpu":
        from ._cpu import cpu_context
        return cpu_context()
    from ._lib import default_context
    return default_context(resolve_device(device))


def column_of_desc(ctx, desc, X, nugget=0.0):
    """``toeplitz_column`` for a descriptor on a context: column 0 of the two-argument build, the one-argument diagonal on top."""
    if not _is_stationary(desc):
        raise NotImplementedError("the Toeplitz path needs a stationary kernel: this one has a DotProduct leaf")
    t = np.array(ctx.kernel_matrix(desc, X, X[:1])[:, 0], dtype=float)
    t[0] = float(desc.one_arg_diagonal()) + float(nugget)
    return t


def toeplitz_column(kernel, X, nugget=0.0, device=None, backend=None):
    """The first column t of ``kernel(X) + nugget I`` for a stationary kernel (a scikit-learn kernel or a ``KernelDesc``) on the points
    X, shape (n,) or (n, 1): ``t[k]``, k >= 1, is the two-argument kernel value between X_k and X_0 as the device builds it
    (``kernel_matrix(desc, X, X[:1])``: bit for bit column 0 of the dense matrix), and ``t[0]`` is the one-argument diagonal, WhiteKernel
    noise included, plus ``nugget``.  X is not checked for uniformity here (``uniform_grid_step``).  NotImplementedError for a kernel
    with a non-stationary leaf (DotProduct), ValueError for more than one feature."""
    X = np.asarray(X, dtype=float)
    if X.ndim == 1:
        X = X[:, None]
    if X.ndim != 2 or X.shape[1] != 1 or X.shape[0] < 1:
        raise ValueError(f"the Toeplitz path takes one feature: X must have shape (n,) or (n, 1), got {X.shape}")
    desc = kernel if isinstance(kernel, KernelDesc) else describe_kernel(kernel, 1)
    return column_of_desc(_context(device, backend), desc, X, nugget)


def toeplitz_max_n(backend=None):
    """The largest n ``toeplitz_gram`` takes: the device's limit (one workgroup holds a generator); none on ``backend='cpu'``."""
    if resolve_backend(backend) == "cpu":
        return None
    from . import _toep_lib
    return _toep_lib.max_n()


def _cpu_gram(t, Z, n_sets):
    """The device's recursion in numpy: the generator in ``numpy.longdouble``, forward substitution and Gram matrices in fp64."""
    ld = np.longdouble
    m, n = t.shape
    cols = Z.shape[1] // n_sets
    info = np.zeros(m, dtype=np.int32)
    t0 = t[:, 0]
    with np.errstate(all="ignore"):
        ok = (t0 > 0) & np.isfinite(t0)
        info[~ok] = 1
        tl = np.where(ok[:, None], t, 1.0).astype(ld)
        u = tl / np.sqrt(tl[:, :1])                                   # (m, n): u[:, i] = L[i, k] for i >= k at step k
        v = u.copy()
        v[:, 0] = 0
        R = np.broadcast_to(Z[None], (m,) + Z.shape).copy()            # the residuals of the forward substitution
        Y = np.zeros_like(R)
        sld = np.zeros(m)
        diag = np.ones((m, n))
        for k in range(n):
            Lkk = u[:, k].astype(float)
            diag[:, k] = Lkk
            y = R[:, k, :] / Lkk[:, None]
            Y[:, k, :] = y
            if k == n - 1:
                break
            R[:, k + 1:, :] -= u[:, k + 1:, None].astype(float) * y[:, None, :]
            rho = v[:, k + 1] / u[:, k]
            fail = ~(np.abs(rho) < 1)
            new = fail & (info == 0)
            info[new] = k + 2
            rho = np.where(fail | (info != 0), ld(0), rho)             # a failed first column idles on
            if np.any(new):
                u[new] = 1
                v[new] = 0
            ic = 1 / np.sqrt((1 - rho) * (1 + rho))
            us = u[:, k:n - 1]                                         # u shifted down by one
            vv = v[:, k + 1:]
            un = (us - rho[:, None] * vv) * ic[:, None]
            v[:, k + 1:] = (vv - rho[:, None] * us) * ic[:, None]
            u[:, k + 1:] = un
        good = info == 0
        sld = np.where(good, np.sum(np.log(np.where(good[:, None], diag, 1.0)), axis=1), np.nan)
        # the device's order (k_gram): 64 partial sums over the rows l, l + 64, ..., then a binary tree over them
        Yp = np.zeros((m, -(-n // 64) * 64, n_sets, cols))
        Yp[:, :n] = Y.reshape(m, n, n_sets, cols)
        Yp = Yp.reshape(m, -1, 64, n_sets, cols)
        P = np.zeros((m, 64, n_sets, cols, cols))
        for blk in range(Yp.shape[1]):
            P += Yp[:, blk, :, :, :, None] * Yp[:, blk, :, :, None, :]
        while P.shape[1] > 1:
            P = P[:, 0::2] + P[:, 1::2]
        G = P[:, 0]
        G[~good] = np.nan
    return G, sld, info


def toeplitz_gram(t, Z, n_sets=1, device=None, backend=None):
    """``(G, sum_log_diag, info)`` of the symmetric Toeplitz matrices with the first columns t, (n,) or (m, n), and the right-hand sides
    Z, (n, n_sets * c) in ``n_sets`` sets of c <= 16 columns: ``G[s] = Z_s^T T^-1 Z_s`` (c x c), ``sum_log_diag = sum_j log L_jj`` of
    ``T = L L^T`` and ``info`` = 0, or the 1-based step at which the pivot of the recursion stops being finite and positive (then G and
    sum_log_diag are NaN).  Shapes: t (n,) gives G (n_sets, c, c) and two scalars; t (m, n) gives (m, n_sets, c, c), (m,), (m,).
    ValueError beyond ``toeplitz_max_n()`` on the device: nothing falls back to a dense evaluation.  On the device the scale of Z is
    free (each column is normalised by a power of two and G scaled back, both exactly), while a positive finite ``t[0]`` outside
    2^-64 .. 2^64 is a ValueError: scale t by a power of 4 instead."""
    t = np.asarray(t, dtype=float)
    single = t.ndim == 1
    t2 = np.ascontiguousarray(t[None] if single else t)
    Z = np.asarray(Z, dtype=float)
    if Z.ndim == 1:
        Z = Z[:, None]
    if t2.ndim != 2 or t2.shape[0] < 1 or t2.shape[1] < 1:
        raise ValueError(f"t must have shape (n,) or (m, n), got {t.shape}")
    n = t2.shape[1]
    n_sets = int(n_sets)
    if Z.ndim != 2 or Z.shape[0] != n or n_sets < 1 or Z.shape[1] < 1 or Z.shape[1] % n_sets:
        raise ValueError(f"Z must have shape ({n}, n_sets * c) with n_sets = {n_sets}, got {Z.shape}")
    cols = Z.shape[1] // n_sets
    if cols > GSUM_MAX_RHS:
        raise ValueError(f"a set takes at most {GSUM_MAX_RHS} columns, got {cols}")
    if resolve_backend(backend) == "cpu":
        G, sld, info = _cpu_gram(t2, Z, n_sets)
    else:
        from . import _toep_lib
        G, sld, info = _toep_lib.default_handle(resolve_device(device)).gram(t2, Z, n_sets)
    if single:
        return G[0], float(sld[0]), int(info[0])
    return G, sld, info
