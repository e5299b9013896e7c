"""The Toeplitz likelihood path: stationary kernels on uniform one-dimensional grids.

With a stationary kernel on a uniform grid, ``R = kernel(X) + nugget I`` is symmetric Toeplitz and fixed by its first column ``t``.  The
Schur (Bareiss) recursion yields the columns of its Cholesky factor one after the other in O(n) each, and a forward substitution runs
beside it: ``G = Z^T T^-1 Z`` and ``sum_j log L_jj`` -- all a likelihood of this package is computed from -- cost O(n^2 c) instead of
O(n^3), and nothing of size n x n is stored.  The generator of the recursion is carried in extended precision (double-double on the
device, ``numpy.longdouble`` on ``backend='cpu'``); a plain fp64 recursion loses several digits on the ill-conditioned matrices the
smooth kernels give.

The result is the likelihood of the exactly Toeplitz matrix of ``t``.  ``kernel(X)`` itself is Toeplitz only up to the last bits of its
entries; on an ill-conditioned matrix that defect, times the condition number, is how far the dense path may sit from this one.

The posterior runs on the same route: the cross-covariance columns of new points ride the forward substitution
beside the residuals (``toeplitz_predict``), and the inverse's first column gives ``diag(T^-1)`` (``toeplitz_inverse_diagonal``) and
with it the leave-one-out predictions (``toeplitz_loo``).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from ._backend import resolve_backend, resolve_device
from ._lib import FAMILY, GSUM_MAX_RHS, KernelDesc
from ._toep_lib import check_grad_method, check_method
from .kernels import describe_kernel

__all__ = ["uniform_grid_step", "toeplitz_column", "toeplitz_gram", "toeplitz_max_n", "toeplitz_panel_width", "toeplitz_inverse_column", "toeplitz_solve",
           "toeplitz_grad", "toeplitz_gradient_columns", "ToeplitzPredict", "toeplitz_predict", "toeplitz_inverse_diagonal", "toeplitz_loo"]


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


def _one_feature(X):
    """X as (n, 1), from (n,) or (n, 1)."""
    X = np.asarray(X, dtype=float)
    if X.ndim == 1:
        X = X[:, None]
    if X.ndim != 2 or X.shape[1] != 1 or X.shape[0] < 1:
        raise ValueError(f"the Toeplitz path takes one feature: X must have shape (n,) or (n, 1), got {X.shape}")
    return X


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
    X = _one_feature(X)
    desc = kernel if isinstance(kernel, KernelDesc) else describe_kernel(kernel, 1)
    return column_of_desc(_context(device, backend), desc, X, nugget)


def toeplitz_max_n(backend=None, method="columns"):
    """The largest n ``toeplitz_gram`` and ``toeplitz_predict`` take with ``method``: the device's limit (one workgroup holds a
    generator; with ``method="blocked"`` the grids of its kernels); none on ``backend='cpu'``."""
    check_method(method)
    if resolve_backend(backend) == "cpu":
        return None
    from . import _toep_lib
    return _toep_lib.max_n(method)


def _cpu_gram(t, Z, n_sets, steps=None):
    """The device's recursion in numpy: the generator in ``numpy.longdouble``, forward substitution and Gram matrices in fp64.
    ``steps``: a dict that receives what the recursion for the inverse's first column needs (``_cpu_inverse_column``): the reflection
    coefficients ``rho`` and the rotations' ``1 / c`` (m, n - 1) and the last pivot ``L[n-1, n-1]`` (m,), all in long double."""
    cols = Z.shape[1] // n_sets
    with np.errstate(all="ignore"):
        Y, sld, info = _cpu_schur(t, Z, steps)
        G = _cpu_ordered_gram(Y, n_sets, cols)
        G[info != 0] = np.nan
    return G, sld, info


def _cpu_ordered_gram(Y, n_sets, cols):
    """G (m, n_sets, cols, cols) of the solved columns Y (m, n, n_sets * cols) in the device's order (k_gram): 64 partial sums over the
    rows l, l + 64, ..., then a binary tree over them."""
    m, n = Y.shape[:2]
    Yp = np.zeros((m, -(-n // 64) * 64, n_sets, cols))
    Yp[:, :n] = Y.reshape(m, n, n_sets, cols)
    Yp = Yp.reshape(m, -1, 64, n_sets, cols)
    P = np.zeros((m, 64, n_sets, cols, cols))
    for blk in range(Yp.shape[1]):
        P += Yp[:, blk, :, :, :, None] * Yp[:, blk, :, :, None, :]
    while P.shape[1] > 1:
        P = P[:, 0::2] + P[:, 1::2]
    return P[:, 0]


def _cpu_schur(t, Z, steps=None):
    """(Y, sum_log_diag, info) of ``_cpu_gram``: the recursion with its forward substitution, Y = L^-1 Z (m, n, ncols) in fp64."""
    ld = np.longdouble
    m, n = t.shape
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
        if steps is not None:
            steps["rho"], steps["ic"] = np.zeros((m, max(n - 1, 0)), dtype=ld), np.ones((m, max(n - 1, 0)), dtype=ld)
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
            if steps is not None:
                steps["rho"][:, k], steps["ic"][:, k] = rho, ic
            us = u[:, k:n - 1]                                         # u shifted down by one
            vv = v[:, k + 1:]
            un = (us - rho[:, None] * vv) * ic[:, None]
            v[:, k + 1:] = (vv - rho[:, None] * us) * ic[:, None]
            u[:, k + 1:] = un
        good = info == 0
        if steps is not None:
            steps["last"] = u[:, n - 1].copy()
        sld = np.where(good, np.sum(np.log(np.where(good[:, None], diag, 1.0)), axis=1), np.nan)
    return Y, sld, info


def _first_columns(t):
    t = np.asarray(t, dtype=float)
    single = t.ndim == 1
    t2 = np.ascontiguousarray(t[None] if single else t)
    if t2.ndim != 2 or t2.shape[0] < 1 or t2.shape[1] < 1:
        raise ValueError(f"t must have shape (n,) or (m, n), got {t.shape}")
    return t2, single


def _rhs_sets(Z, n, n_sets):
    """(Z (n, n_sets * c), n_sets, c) of the right-hand sides of ``toeplitz_gram`` and ``toeplitz_grad``; (n,) is one column."""
    Z = np.asarray(Z, dtype=float)
    if Z.ndim == 1:
        Z = Z[:, None]
    n_sets = int(n_sets)
    if Z.ndim != 2 or Z.shape[0] != n or n_sets < 1 or Z.shape[1] < 1 or Z.shape[1] % n_sets:
        raise ValueError(f"Z must have shape ({n}, n_sets * c) with n_sets = {n_sets}, got {Z.shape}")
    cols = Z.shape[1] // n_sets
    if cols > GSUM_MAX_RHS:
        raise ValueError(f"a set takes at most {GSUM_MAX_RHS} columns, got {cols}")
    return Z, n_sets, cols


def toeplitz_panel_width():
    """The columns of L per panel of ``method="panel"`` on the device (needs no device): a compile-time constant of the library."""
    from . import _toep_lib
    return _toep_lib.panel_width()


def toeplitz_gram(t, Z, n_sets=1, device=None, backend=None, method="columns"):
    """``(G, sum_log_diag, info)`` of the symmetric Toeplitz matrices with the first columns t, (n,) or (m, n), and the right-hand sides
    Z, (n, n_sets * c) in ``n_sets`` sets of c <= 16 columns: ``G[s] = Z_s^T T^-1 Z_s`` (c x c), ``sum_log_diag = sum_j log L_jj`` of
    ``T = L L^T`` and ``info`` = 0, or the 1-based step at which the pivot of the recursion stops being finite and positive (then G and
    sum_log_diag are NaN).  Shapes: t (n,) gives G (n_sets, c, c) and two scalars; t (m, n) gives (m, n_sets, c, c), (m,), (m,).
    ValueError beyond ``toeplitz_max_n()`` on the device: nothing falls back to a dense evaluation.  On the device the scale of Z is
    free (each column is normalised by a power of two and G scaled back, both exactly), while a positive finite ``t[0]`` outside
    2^-64 .. 2^64 is a ValueError: scale t by a power of 4 instead.
    ``method="columns"`` keeps the residual columns beside the recursion, a few per workgroup, and repeats the recursion for every
    further few; ``method="panel"`` runs one recursion per first column in panels of
    ``toeplitz_panel_width()`` columns of L and applies each panel to all columns at once on the matrix unit: the schedule for many
    sets.  Same arithmetic per entry, cut into panels: G agrees to the accuracy of either, ``sum_log_diag`` and ``info`` bit for
    bit.  ``method="blocked"`` splits each panel's recursion into a serial lead on the rows under the pivot
    and tiles that replay its coefficients on all rows at once, with the generator in device memory: bit for bit the panel route's
    results, and the one schedule beyond ``toeplitz_max_n()``, up to ``toeplitz_max_n(method="blocked")``.  ``backend='cpu'`` has
    one code for all three."""
    check_method(method)
    t2, single = _first_columns(t)
    Z, n_sets, cols = _rhs_sets(Z, t2.shape[1], n_sets)
    if resolve_backend(backend) == "cpu":
        G, sld, info = _cpu_gram(t2, Z, n_sets)
    else:
        from . import _toep_lib
        G, sld, info = _toep_lib.default_handle(resolve_device(device)).gram(t2, Z, n_sets, method)
    if single:
        return G[0], float(sld[0]), int(info[0])
    return G, sld, info


# ---- the gradient pieces ---------------------------------------------------------------------------------------

def _cpu_inverse_column(steps, info):
    """x = T^-1 e_0 (m, n) in long double from the recursion's reflection coefficients: Levinson's recursion in its normalised form.
    A and B start as e_0 / sqrt(t_0) -- here e_0, the factor is taken off with the last pivot -- and a step rotates (A, shift(B)) as
    the generator was rotated; A ends as the last row of L^-1 reversed, times sqrt(t_0)."""
    ld = np.longdouble
    rho, ic, last = steps["rho"], steps["ic"], steps["last"]
    m, n = rho.shape[0], rho.shape[1] + 1
    A = np.zeros((m, n), dtype=ld)
    A[:, 0] = 1
    B = A.copy()
    for k in range(1, n):
        r, c = rho[:, k - 1, None], ic[:, k - 1, None]
        Bs = np.concatenate([np.zeros((m, 1), dtype=ld), B[:, :k]], axis=1)
        Ak = A[:, :k + 1]
        A[:, :k + 1], B[:, :k + 1] = (Ak - r * Bs) * c, (Bs - r * Ak) * c
    x = A / (last * steps["root"])[:, None]
    x[info != 0] = np.nan
    return x


def _lower_times(a, w):
    """L(a) w, L(a) the lower-triangular Toeplitz matrix of the first column a."""
    return np.convolve(a, w)[:len(a)]


def _lower_t_times(a, z):
    """L(a)^T z."""
    return np.convolve(a, z[::-1])[:len(a)][::-1]


def _cpu_solve_columns(x, Z):
    """alpha = T^-1 Z (n, c) in long double by the Gohberg-Semencul formula, x = T^-1 e_0."""
    ld = np.longdouble
    n = len(x)
    xt = np.concatenate([[ld(0)], x[:0:-1]])
    out = np.empty((n, Z.shape[1]), dtype=ld)
    for c in range(Z.shape[1]):
        z = Z[:, c].astype(ld)
        out[:, c] = (_lower_times(x, _lower_t_times(x, z)) - _lower_times(xt, _lower_t_times(xt, z))) / x[0]
    return out


def _cpu_diagonal_sums(x):
    """s_d = sum of the d-th diagonal of T^-1 = (1 / x_0) sum_m (n - d - 2 m) x_m x_{m+d} (long double)."""
    ld = np.longdouble
    n = len(x)
    m = np.arange(n, dtype=ld)
    return np.array([np.sum((n - d - 2 * m[:n - d]) * x[:n - d] * x[d:]) for d in range(n)], dtype=ld) / x[0]


_cpu_last = {}                                                         # see _cpu_pieces


def _cpu_pieces(t, dt, Z, n_sets, want):
    """(G, sld, info, x, alpha, trace, H) of ``backend='cpu'``: ``want`` names what beyond the first three is computed (None otherwise).
    Everything in ``numpy.longdouble``, rounded to fp64 at the end.  The recursion of the last first columns and alpha of the last
    right-hand sides are kept, so that ``toeplitz_inverse_column``, ``toeplitz_solve`` and ``toeplitz_grad`` of one problem run them once."""
    ld = np.longdouble
    m, n = t.shape
    key = (t.shape, t.tobytes())
    memo = _cpu_last if _cpu_last.get("key") == key else None          # the last first columns' recursion: x, alpha per Z
    G = sld = None
    with np.errstate(all="ignore"):
        if memo is None or "trace" in want:
            steps = {}
            G, sld, info = _cpu_gram(t, Z, n_sets, steps)
        if memo is None:
            steps["root"] = np.sqrt(np.where(info == 0, t[:, 0], 1.0).astype(ld))
            x = _cpu_inverse_column(steps, info)
            bad = (info == 0) & ~np.all(np.isfinite(x.astype(float)), axis=1)
            info[bad] = n + 1
            x[info != 0] = np.nan
            _cpu_last.clear()
            _cpu_last.update(key=key, x=x, info=info.copy(), alpha={})
            memo = _cpu_last
        x, info = memo["x"], memo["info"].copy()
        good = info == 0
        if G is not None:
            G[~good], sld[~good] = np.nan, np.nan
        alpha = trace = H = None
        if "alpha" in want or "H" in want:
            zkey = (Z.shape, Z.tobytes())
            if zkey not in memo["alpha"]:
                alpha = np.full((m, n, Z.shape[1]), np.nan, dtype=ld)
                for i in np.flatnonzero(good):
                    alpha[i] = _cpu_solve_columns(x[i], Z)
                memo["alpha"].clear()
                memo["alpha"][zkey] = alpha
            alpha = memo["alpha"][zkey]
        if "trace" in want:
            P = dt.shape[1]
            trace = np.full((m, P), np.nan)
            for i in np.flatnonzero(good):
                s = _cpu_diagonal_sums(x[i])
                w = np.full(n, ld(2))
                w[0] = 1
                trace[i] = [float(np.sum(w * dt[i, p].astype(ld) * s)) for p in range(P)]
        if "H" in want:
            P, cols = dt.shape[1], Z.shape[1] // n_sets
            H = np.full((m, n_sets, P, cols, cols), np.nan)
            for i in np.flatnonzero(good):
                for p in range(P):
                    d = dt[i, p].astype(ld)
                    Q = np.stack([_lower_times(d, alpha[i, :, c]) + _lower_t_times(d, alpha[i, :, c]) - d[0] * alpha[i, :, c]
                                  for c in range(Z.shape[1])], axis=1)
                    for s_ in range(n_sets):
                        sl = slice(s_ * cols, (s_ + 1) * cols)
                        Hs = alpha[i][:, sl].T @ Q[:, sl]
                        H[i, s_, p] = np.triu(Hs) + np.triu(Hs, 1).T
    return G, sld, info, x.astype(float), None if alpha is None else alpha.astype(float), trace, H


def toeplitz_inverse_column(t, device=None, backend=None, method="columns"):
    """``(x, info)``: the first column ``x = T^-1 e_0`` of the inverse of the symmetric Toeplitz matrices with the first columns t, (n,)
    or (m, n), and ``info`` as ``toeplitz_gram`` gives it, or n + 1 where the recursion went through but x is not finite.  x is NaN where
    info is not 0.  By Gohberg and Semencul x fixes the whole inverse.  ``method="blocked"``: the blocked
    route's recursion and Levinson's replay on tiles, bit for bit the default's x, up to ``toeplitz_max_n(method="blocked")``; the
    same keyword on ``toeplitz_solve``, ``toeplitz_grad``, ``toeplitz_inverse_diagonal`` and ``toeplitz_loo``.  There is no panel
    route from x on: ``"panel"`` is a ValueError.  ``backend='cpu'`` has one code for both."""
    check_grad_method(method)
    t2, single = _first_columns(t)
    if resolve_backend(backend) == "cpu":
        _, _, info, x, _, _, _ = _cpu_pieces(t2, None, np.zeros((t2.shape[1], 1)), 1, ())
    else:
        from . import _toep_lib
        x, _, info = _toep_lib.default_handle(resolve_device(device)).solve(t2, None, want_x=True, method=method)
    return (x[0], int(info[0])) if single else (x, info)


def toeplitz_solve(t, Z, device=None, backend=None, method="columns"):
    """``(alpha, info)``: ``alpha = T^-1 Z`` for the first columns t, (n,) or (m, n), and the right-hand sides Z, (n,) or (n, c): alpha
    is (n, c) or (m, n, c), NaN where info is not 0.  Four triangular Toeplitz products per column (Gohberg-Semencul), O(n^2 c).
    ``method``: see ``toeplitz_inverse_column``."""
    check_grad_method(method)
    t2, single = _first_columns(t)
    Z = np.asarray(Z, dtype=float)
    if Z.ndim == 1:
        Z = Z[:, None]
    n = t2.shape[1]
    if Z.ndim != 2 or Z.shape[0] != n or Z.shape[1] < 1:
        raise ValueError(f"Z must have shape ({n}, c), got {Z.shape}")
    if resolve_backend(backend) == "cpu":
        _, _, info, _, alpha, _, _ = _cpu_pieces(t2, None, Z, 1, ("alpha",))
    else:
        from . import _toep_lib
        _, alpha, info = _toep_lib.default_handle(resolve_device(device)).solve(t2, Z, want_x=False, method=method)
    return (alpha[0], int(info[0])) if single else (alpha, info)


def toeplitz_grad(t, dt, Z, n_sets=1, device=None, backend=None, method="columns"):
    """``(G, sum_log_diag, info, trace, H)``: ``toeplitz_gram``'s three and, for the derivative columns dt, (P, n) or (m, P, n) -- dT_p
    is the symmetric Toeplitz matrix of ``dt[p]`` -- ``trace[p] = tr(T^-1 dT_p)`` and ``H[s, p] = alpha_s^T dT_p alpha_s`` with
    ``alpha_s = T^-1 Z_s`` (exactly symmetric): what ``lml_grad_from_gram`` takes.  Shapes: t (n,) gives trace (P,) and H (n_sets, P, c,
    c); t (m, n) gives (m, P) and (m, n_sets, P, c, c).  Where info is not 0 (n + 1: the inverse's first column is not finite) all
    outputs are NaN.  G, sum_log_diag and info are bit for bit ``toeplitz_gram``'s, with ``method="blocked"`` (see
    ``toeplitz_inverse_column``) those of ``toeplitz_gram(method="blocked")``."""
    check_grad_method(method)
    t2, single = _first_columns(t)
    m, n = t2.shape
    dt = np.asarray(dt, dtype=float)
    dt3 = np.ascontiguousarray(dt[None] if (single and dt.ndim == 2) else dt)
    if dt3.ndim != 3 or dt3.shape[0] != m or dt3.shape[2] != n:
        raise ValueError(f"dt must have shape (P, {n}) for one first column or ({m}, P, {n}), got {dt.shape}")
    if dt3.shape[1] < 1:
        raise ValueError("dt must hold at least one derivative column (P >= 1)")
    Z, n_sets, cols = _rhs_sets(Z, n, n_sets)
    if resolve_backend(backend) == "cpu":
        G, sld, info, _, _, trace, H = _cpu_pieces(t2, dt3, Z, n_sets, ("trace", "H"))
    else:
        from . import _toep_lib
        G, sld, info, trace, H = _toep_lib.default_handle(resolve_device(device)).grad(t2, dt3, Z, n_sets, method)
    if single:
        return G[0], float(sld[0]), int(info[0]), trace[0], H[0]
    return G, sld, info, trace, H


def toeplitz_gradient_columns(kernel, X, theta=None, block=256):
    """``dt`` (P, n): column 0 of scikit-learn's ``kernel(X, eval_gradient=True)[1]`` in theta order, for a stationary scikit-learn
    kernel on the points X, shape (n,) or (n, 1); ``theta`` (log-transformed, default the kernel's own) is set on a clone.  Evaluated on
    the host in blocks of ``block`` points together with X_0, so nothing n x n is formed; the entries are entrywise functions of the
    pair, so this is the dense column bit for bit.  ``dt[p, 0]`` is the diagonal's derivative: a free WhiteKernel contributes its noise
    level, a nugget nothing.  Refuses what ``toeplitz_column`` refuses."""
    from sklearn.base import clone
    X = _one_feature(X)
    if not _is_stationary(describe_kernel(kernel, 1)):
        raise NotImplementedError("the Toeplitz path needs a stationary kernel: this one has a DotProduct leaf")
    if theta is not None:
        kernel = clone(kernel)
        kernel.theta = np.asarray(theta, dtype=float)
    n, P = X.shape[0], kernel.n_dims
    out = np.empty((P, n))
    if P == 0:
        return out
    out[:, 0] = kernel(X[:1], eval_gradient=True)[1][0, 0, :]
    for a in range(1, n, block):
        b = min(n, a + block)
        out[:, a:b] = kernel(np.vstack([X[:1], X[a:b]]), eval_gradient=True)[1][1:, 0, :].T
    return out


# ---- the posterior pieces ---------------------------------------------------------------------------------------

Y_BUDGET = 256 << 20                                                   # bytes of solved columns one device call of toeplitz_predict keeps

ToeplitzPredict = namedtuple("ToeplitzPredict", ["quad", "cross", "cov", "G", "sum_log_diag", "info"])
ToeplitzPredict.__doc__ = """What a posterior at q new points takes from T: ``quad`` (q,) = diag(K^T T^-1 K), ``cross`` (q, c) = K^T T^-1 Z,
``cov`` (q, q) = K^T T^-1 K or None, ``G`` (c, c) = Z^T T^-1 Z, ``sum_log_diag`` and ``info`` as ``toeplitz_gram`` gives them."""


def _cpu_predict(t, K, Z, want_cov):
    """``_cpu_gram``'s recursion on the columns [K | Z], keeping the solved columns Y: quad and cross summed in long double, cov as
    Y^T Y in fp64 (summed over the rows in order), G in the device's order."""
    ld = np.longdouble
    q, c = K.shape[1], Z.shape[1]
    with np.errstate(all="ignore"):
        Y, sld, info = _cpu_schur(t[None], np.concatenate([K, Z], axis=1))
        Y = Y[0]
        Yk, Yz = Y[:, :q], Y[:, q:]
        Yl = Yk.astype(ld)
        quad = np.sum(Yl * Yl, axis=0).astype(float)
        cross = (Yl.T @ Yz.astype(ld)).astype(float).reshape(q, c)
        cov = None
        if want_cov:                                                   # row by row, as the device accumulates it: an entry's sum does not
            cov = np.zeros((q, q))                                     # depend on the other columns or on their order
            for k in range(Yk.shape[0]):
                cov += Yk[k][:, None] * Yk[k][None, :]
        G = _cpu_ordered_gram(np.ascontiguousarray(Yz)[None], 1, c)[0, 0] if c else np.empty((0, 0))
        if info[0] != 0:
            for a in (quad, cross, cov, G):
                if a is not None:
                    a[...] = np.nan
    return quad, cross, cov, G, float(sld[0]), int(info[0])


def predict_chunk(n, c=0):
    """The most new points one device call of ``toeplitz_predict`` takes at order n beside c residual columns: what keeps the solved
    columns, n (q + c) doubles, within 256 MB."""
    return max(1, Y_BUDGET // (8 * int(n)) - int(c))


def toeplitz_predict(t, K, Z=None, want_cov=False, chunk=None, device=None, backend=None, method="columns"):
    """``ToeplitzPredict(quad, cross, cov, G, sum_log_diag, info)`` of the symmetric Toeplitz matrix with the first column t, (n,), the
    cross-covariance columns K, (n, q) -- column j holds the covariances of the n grid points with new point j -- and the residual
    columns Z, (n, c) with c <= 16, (n,) or None: ``quad[j] = K_j^T T^-1 K_j``, ``cross = K^T T^-1 Z`` (q, c), ``cov = K^T T^-1 K``
    (q, q; only with ``want_cov``, otherwise None; exactly symmetric) and ``G = Z^T T^-1 Z`` (c, c), bit for bit ``toeplitz_gram``'s.
    Nothing n x n is formed: the columns ride the forward substitution of the Schur recursion.  ``chunk`` is the largest number of
    new points per device call (default ``predict_chunk(n, c)``); the results do not depend on it bit for bit.  ``want_cov`` needs all
    q points in one call: ValueError, naming the limit, otherwise.  Where ``info`` is not 0 every array is NaN.
    ``method="panel"``: all columns of a call ride one recursion (``toeplitz_gram``); ``chunk`` then only bounds the memory.
    ``method="blocked"``: the panel route's results from the tiled recursion, for n up to ``toeplitz_max_n(method="blocked")``."""
    check_method(method)
    t = np.asarray(t, dtype=float)
    if t.ndim != 1 or t.size < 1:
        raise ValueError(f"t must have shape (n,), got {t.shape}")
    n = t.size
    K = np.asarray(K, dtype=float)
    if K.ndim == 1:
        K = K[:, None]
    if K.ndim != 2 or K.shape[0] != n or K.shape[1] < 1:
        raise ValueError(f"K must have shape ({n}, q) with q >= 1, got {K.shape}")
    Z = np.zeros((n, 0)) if Z is None else np.asarray(Z, dtype=float)
    if Z.ndim == 1:
        Z = Z[:, None]
    if Z.ndim != 2 or Z.shape[0] != n:
        raise ValueError(f"Z must have shape ({n}, c), got {Z.shape}")
    q, c = K.shape[1], Z.shape[1]
    if c > GSUM_MAX_RHS:
        raise ValueError(f"Z takes at most {GSUM_MAX_RHS} columns, got {c}")
    limit = predict_chunk(n, c)
    if chunk is None:
        chunk = limit
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    if want_cov and q > chunk:
        raise ValueError(f"want_cov takes all new points in one call: q = {q} exceeds the limit of {chunk} points per call "
                         f"(n = {n}: {limit} keep the solved columns within {Y_BUDGET >> 20} MB)")
    if resolve_backend(backend) == "cpu":
        call = lambda Kc, cov: _cpu_predict(t, Kc, Z, cov)  # noqa: E731
    else:
        from . import _toep_lib
        handle = _toep_lib.default_handle(resolve_device(device))
        call = lambda Kc, cov: handle.predict(t, Kc, Z, cov, method)  # noqa: E731
    if q <= chunk:
        return ToeplitzPredict(*call(K, want_cov))
    quad, cross = np.empty(q), np.empty((q, c))
    for lo in range(0, q, chunk):
        hi = min(q, lo + chunk)
        quad[lo:hi], cross[lo:hi], _, G, sld, info = call(K[:, lo:hi], False)
    return ToeplitzPredict(quad, cross, None, G, sld, info)


def _cpu_inverse_diagonal(t):
    """(p (m, n), info) of ``backend='cpu'``: the long-double running sums of (x_r - x_{n-r}) (x_r + x_{n-r}) over x_0, x the inverse's
    first column of ``_cpu_pieces`` (whose memo this reuses), rounded to fp64 at the end."""
    ld = np.longdouble
    m, n = t.shape
    _, _, info, _, _, _, _ = _cpu_pieces(t, None, np.zeros((n, 1)), 1, ())
    x = _cpu_last["x"]
    with np.errstate(all="ignore"):
        xn = np.concatenate([np.zeros((m, 1), dtype=ld), x[:, :0:-1]], axis=1)             # x_{n-r}, 0 at r = 0
        p = (np.cumsum((x - xn) * (x + xn), axis=1) / x[:, :1]).astype(float)
    p[info != 0] = np.nan
    return p, info


def toeplitz_inverse_diagonal(t, device=None, backend=None, method="columns"):
    """``(p, info)``: ``p = diag(T^-1)`` of the symmetric Toeplitz matrices with the first columns t, (n,) or (m, n), from the inverse's
    first column x by Gohberg and Semencul: ``p_i = (1 / x_0) sum_{r <= i} (x_r^2 - x_{n-r}^2)`` with ``x_n = 0``.  The sums cancel
    heavily on an ill-conditioned T and run in extended precision throughout.  ``info`` as ``toeplitz_inverse_column``; p is NaN where
    it is not 0.  ``method``: see ``toeplitz_inverse_column``."""
    check_grad_method(method)
    t2, single = _first_columns(t)
    if resolve_backend(backend) == "cpu":
        p, info = _cpu_inverse_diagonal(t2)
    else:
        from . import _toep_lib
        p, _, info = _toep_lib.default_handle(resolve_device(device)).loo(t2, None, method)
    return (p[0], int(info[0])) if single else (p, info)


def toeplitz_loo(t, y, mean=0.0, device=None, backend=None, method="columns"):
    """The ``LooResult`` (``gsum_amd.loo``) of the curves y, (n,) or (n, n_curves), under N(mean, T), T the symmetric Toeplitz matrix
    with the first column t, (n,): ``LooFactor.loo``'s formulas with ``a = T^-1 (y - mean)`` (``toeplitz_solve``) and ``p = diag(T^-1)``
    (``toeplitz_inverse_diagonal``), both from one recursion; nothing n x n is formed.  ``mean`` is a scalar or (n,).
    numpy.linalg.LinAlgError where T is not positive definite.  ``method``: see ``toeplitz_inverse_column``."""
    from .loo import LooResult
    check_grad_method(method)
    t = np.asarray(t, dtype=float)
    if t.ndim != 1 or t.size < 1:
        raise ValueError(f"t must have shape (n,), got {t.shape}")
    n = t.size
    y = np.asarray(y, dtype=float)
    if y.ndim not in (1, 2) or y.shape[0] != n or y.size == 0:
        raise ValueError(f"y must be ({n},) or ({n}, n_curves), got {y.shape}")
    mean = np.asarray(mean, dtype=float)
    if mean.shape not in ((), (n,)):
        raise ValueError(f"mean must be a scalar or ({n},), got {mean.shape}")
    r = (y.T - mean).T.reshape(n, -1)
    if resolve_backend(backend) == "cpu":
        p, info = _cpu_inverse_diagonal(t[None])
        _, _, _, _, a, _, _ = _cpu_pieces(t[None], None, r, 1, ("alpha",))
    else:
        from . import _toep_lib
        p, a, info = _toep_lib.default_handle(resolve_device(device)).loo(t[None], r, method)
    if info[0] != 0:
        raise np.linalg.LinAlgError("Matrix is not positive definite")
    p, a = p[0], a[0].reshape(y.shape)
    pc = p if y.ndim == 1 else p[:, None]
    return LooResult(mean=y - a / pc, var=1.0 / p, error=a / np.sqrt(pc), logpdf=-0.5 * np.log(2 * np.pi) + 0.5 * np.log(pc) - 0.5 * a * a / pc,
                     precision_diag=p)
