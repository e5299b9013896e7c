"""The banded likelihood path: short-range kernels on sorted one-dimensional points.

A stationary kernel whose exponential underflows -- ``exp(-r^2 / 2 l^2)`` is exactly 0.0 from r = 38.6 l on -- gives, on sorted points,
a kernel matrix that is banded in fp64.  A band Cholesky of half-bandwidth b costs n b^2 operations on n (b + 1) doubles instead of
n^3 / 3 on n^2, and the points need not be uniform (the one case ``structure="toeplitz"`` cannot take).

Band layout (LAPACK lower band storage, ``scipy.linalg.cholesky_banded(..., lower=True)``): ``AB[k, j] = A[j + k, j]``, shape
``(b + 1, n)``; entries with ``j + k >= n`` are ignored on input and zero on output.

PREMISE of the width search.  ``banded_halfwidth`` looks at ``banded_max_halfwidth() + 1`` off-diagonals and nothing else.  That the
entries beyond them are exact zeros as well follows from the kernel not increasing with ``|x_i - x_j|`` on sorted points: true for
RBF, Matern and RationalQuadratic leaves under Sum / Product / Exponentiation with ConstantKernel and WhiteKernel, not for
ExpSineSquared or DotProduct leaves, which are refused unevaluated.

The result is the likelihood of the band.  Where the premise holds it is the matrix itself, entry for entry.
"""
from __future__ import annotations

import numpy as np

from ._backend import resolve_backend, resolve_device
from ._lib import FAMILY, GSUM_MAX_RHS, KernelDesc
from .kernels import describe_kernel

__all__ = ["sorted_points", "banded_halfwidth", "banded_matrix", "banded_gram", "banded_forward", "banded_max_halfwidth"]

_SEARCH = 255                    # off-diagonals (plus one) backend='cpu' searches: the device library's limit, so both answer alike
_LN2 = 0.69314718055994530942


def sorted_points(X):
    """X as (n, 1), from (n,) or (n, 1), after checking that it has one feature and is finite and non-decreasing (duplicates are
    allowed).  ValueError, naming the first offending index, otherwise: nothing is sorted silently."""
    X = np.asarray(X, dtype=float)
    if X.ndim == 2 and X.shape[1] != 1:
        raise ValueError(f"sorted points have one feature, X has {X.shape[1]}")
    if X.ndim == 1:
        X = X[:, None]
    if X.ndim != 2 or X.shape[0] < 1:
        raise ValueError(f"X must have shape (n,) or (n, 1) with n >= 1, got {np.shape(X)}")
    if not np.all(np.isfinite(X)):
        raise ValueError(f"X is not finite at index {int(np.argmin(np.isfinite(X[:, 0])))}")
    down = np.diff(X[:, 0]) < 0
    if np.any(down):
        raise ValueError(f"X is not sorted: X[{int(np.argmax(down)) + 1}] is below X[{int(np.argmax(down))}] (sort the points and the curves first)")
    return X


def banded_max_halfwidth(backend=None):
    """The widest half-bandwidth the device takes (a constant of libgsum_band.so; needs no device); None on ``backend='cpu'``."""
    if resolve_backend(backend) == "cpu":
        return None
    from . import _band_lib
    return _band_lib.max_halfwidth()


def _descs(kernel):
    """(descriptors, single) of a kernel, a descriptor or a list of either, each checked for the premise."""
    single = not isinstance(kernel, (list, tuple))
    out = []
    for k in ([kernel] if single else kernel):
        d = k if isinstance(k, KernelDesc) else describe_kernel(k, 1)
        check_monotone(d)
        out.append(d)
    if not out:
        raise ValueError("no kernel given")
    return out, single


def check_monotone(desc):
    """NotImplementedError for a descriptor with an ExpSineSquared or DotProduct leaf: not monotone in distance, never evaluated."""
    fams = [desc.leaf[i].family for i in range(desc.n_leaves)] if desc.is_tree else [desc.family]
    for f in fams:
        if f in (FAMILY["expsine"], FAMILY["dot"]):
            name = "ExpSineSquared" if f == FAMILY["expsine"] else "DotProduct"
            raise NotImplementedError(f"the banded path needs a kernel that is not increasing with distance: a {name} leaf is not monotone in distance")


def _handle(device):
    from . import _band_lib
    return _band_lib.default_handle(resolve_device(device))


def _cpu_off_diagonals(desc, X, kmax):
    """(kmax, n): row k - 1 holds K(x_{j+k}, x_j), j + k < n, zeros beyond -- the two-argument form, as the cpu backend builds it."""
    from ._cpu import kernel_matrix
    n = X.shape[0]
    out = np.zeros((kmax, n))
    rows = 512
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        c0 = max(0, r0 - kmax)
        K = kernel_matrix(desc, X[r0:r1], X[c0:r1])                    # rows r0 .. r1, columns c0 .. r1
        for k in range(1, kmax + 1):
            i = np.arange(max(r0, k), r1)                              # rows with a column i - k >= 0
            i = i[i - k >= c0]
            if i.size:
                out[k - 1, i - k] = K[i - r0, i - k - c0]
    return out


def _widths(descs, X, nugget, device, backend):
    if resolve_backend(backend) == "cpu":
        w = []
        for d in descs:
            off = _cpu_off_diagonals(d, X, _SEARCH + 1)
            nz = np.nonzero(np.any((off.view(np.uint64) << np.uint64(1)) != 0, axis=1))[0]
            w.append(int(nz[-1]) + 1 if nz.size else 0)
        return np.array(w, dtype=np.int64), _SEARCH
    h = _handle(device)
    from . import _band_lib
    return h.width(descs, X[:, 0], nugget).astype(np.int64), _band_lib.max_halfwidth()


def _checked_widths(descs, X, nugget, device, backend):
    w, limit = _widths(descs, X, nugget, device, backend)
    if np.any(w > limit):
        i = int(np.argmax(w > limit))
        raise ValueError(f"half-bandwidth exceeds {limit}: kernel {i} has a nonzero entry {limit + 1} off the diagonal (an additive constant, or a "
                         "length scale too long for these points)")
    return w


def banded_halfwidth(kernel, X, nugget=0.0, device=None, backend=None):
    """The half-bandwidth b of ``kernel(X) + nugget I`` on the sorted points X: the smallest b such that every entry ``K[i, i + k]``,
    ``1 <= k <= banded_max_halfwidth() + 1``, with bits other than +-0 has ``k <= b`` (NaN and Inf count as nonzero).  An int, or an
    array for a list of kernels or descriptors.  ValueError ("half-bandwidth exceeds ...") when there is no such b within the limit
    (an additive constant, a kernel too long-ranged), NotImplementedError for an ExpSineSquared or DotProduct leaf ("not monotone in
    distance"; see the module's PREMISE)."""
    descs, single = _descs(kernel)
    w = _checked_widths(descs, sorted_points(X), nugget, device, backend)
    return int(w[0]) if single else w


def _cpu_build(descs, X, nugget, b):
    n = X.shape[0]
    AB = np.zeros((len(descs), b + 1, n))
    for i, d in enumerate(descs):
        if b:
            AB[i, 1:] = _cpu_off_diagonals(d, X, b)
        AB[i, 0] = float(d.one_arg_diagonal()) + float(nugget)
    return AB


def banded_matrix(kernel, X, nugget=0.0, halfwidth=None, device=None, backend=None):
    """The band AB of ``kernel(X) + nugget I`` on the sorted points X: ``(b + 1, n)``, or ``(m, b + 1, n)`` for a list of kernels or
    descriptors (all at the widest member's b).  ``AB[k, j]``, k >= 1, is the two-argument kernel value between x_{j+k} and x_j as the
    backend builds it (on the device bit for bit entry ``[j + k, j]`` of ``kernel_matrix(desc, X, X)``); ``AB[0, j]`` is the
    one-argument diagonal, WhiteKernel noise included, plus ``nugget``.  ``halfwidth=None`` takes ``banded_halfwidth``; a given one is
    used as it is (whatever the kernel has beyond it is dropped)."""
    descs, single = _descs(kernel)
    X = sorted_points(X)
    if halfwidth is None:
        b = int(np.max(_checked_widths(descs, X, nugget, device, backend)))
    else:
        b = int(halfwidth)
        if b < 0:
            raise ValueError(f"halfwidth must be >= 0, got {halfwidth}")
    if resolve_backend(backend) == "cpu":
        AB = _cpu_build(descs, X, nugget, b)
    else:
        AB = _handle(device).build(descs, X[:, 0], nugget, b)
    return AB[0] if single else AB


def _bands(AB, name="AB"):
    AB = np.asarray(AB, dtype=float)
    single = AB.ndim == 2
    A3 = np.ascontiguousarray(AB[None] if single else AB)
    if A3.ndim != 3 or min(A3.shape) < 1:
        raise ValueError(f"{name} must have shape (b + 1, n) or (m, b + 1, n), got {AB.shape}")
    return A3, single


def _rhs_sets(Z, n, n_sets):
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


def _cpu_factor(AB):
    """(L (m, b + 1, n), info (m,)): LAPACK's dpbtrf per matrix; a pivot that is not finite counts as not positive."""
    from scipy.linalg.lapack import dpbtrf
    m, b1, n = AB.shape
    L = np.zeros_like(AB)
    info = np.zeros(m, dtype=np.int32)
    for i in range(m):
        ab = AB[i].copy()
        for k in range(1, b1):
            ab[k, max(n - k, 0):] = 0.0
        with np.errstate(all="ignore"):
            c, inf_ = dpbtrf(ab, lower=1)
        if inf_ < 0:
            raise ValueError(f"dpbtrf refused argument {-inf_}")
        L[i] = c
        for k in range(1, b1):
            L[i, k, max(n - k, 0):] = 0.0
        bad = np.nonzero(~(np.isfinite(c[0]) & (c[0] > 0)))[0]
        first = int(bad[0]) + 1 if bad.size else 0
        info[i] = inf_ if inf_ > 0 and (first == 0 or inf_ <= first) else first
    return L, info


def _cpu_forward(L, Z):
    """Y (m, n, ncols) = L^-1 Z by forward substitution in numpy, row by row."""
    m, b1, n = L.shape
    Y = np.zeros((m, n, Z.shape[1]))
    with np.errstate(all="ignore"):
        for i in range(n):
            k = np.arange(1, min(b1 - 1, i) + 1)
            acc = np.broadcast_to(Z[i], (m, Z.shape[1]))
            if k.size:
                acc = acc - np.einsum("mk,mkc->mc", L[:, k, i - k], Y[:, i - k, :])
            Y[:, i, :] = acc / L[:, 0, i][:, None]
    return Y


def _cpu_sld(diag):
    """sum log L_jj with the binary exponents summed as integers (the device's sum: a diagonal of powers of two gives it exactly)."""
    with np.errstate(all="ignore"):
        f, e = np.frexp(diag)
        low = f < np.sqrt(0.5)
        f = np.where(low, 2.0 * f, f)
        e = e - low
        return float(e.sum()) * _LN2 + float(np.sum(np.log(f)))


def _cpu_gram(AB, Z, n_sets, cols):
    m, _, n = AB.shape
    L, info = _cpu_factor(AB)
    ok = info == 0
    G = np.full((m, n_sets, cols, cols), np.nan)
    sld = np.full(m, np.nan)
    if np.any(ok):
        Y = _cpu_forward(L[ok], Z).reshape(int(ok.sum()), n, n_sets, cols)
        G[ok] = np.einsum("mnsa,mnsb->msab", Y, Y)
        sld[ok] = [_cpu_sld(L[i, 0]) for i in np.nonzero(ok)[0]]
    return G, sld, info, L


def banded_gram(AB, Z, n_sets=1, return_factor=False, device=None, backend=None):
    """``(G, sum_log_diag, info[, L])`` of the symmetric band matrices AB, ``(b + 1, n)`` or ``(m, b + 1, n)``, and the right-hand sides
    Z, ``(n, n_sets * c)`` in ``n_sets`` sets of c <= 16 columns: ``G[s] = Z_s^T A^-1 Z_s`` (c x c), ``sum_log_diag = sum_j log L_jj`` of
    the band Cholesky ``A = L L^T`` and ``info`` = LAPACK ``dpbtrf``'s: 0, or the 1-based order of the first leading minor whose pivot is
    not finite and positive (then G and sum_log_diag are NaN).  ``return_factor``: L in the band layout as well.  Shapes: AB
    ``(b + 1, n)`` gives G ``(n_sets, c, c)`` and two scalars; ``(m, b + 1, n)`` gives ``(m, n_sets, c, c)``, ``(m,)``, ``(m,)``.
    ValueError beyond ``banded_max_halfwidth()`` on the device: nothing falls back.  On the device every result of a matrix is bitwise
    reproducible, whatever else the call carries and whatever all-zero diagonals the band is stored with; ``backend='cpu'`` is
    ``dpbtrf`` (``scipy.linalg.cholesky_banded``'s routine) and a numpy substitution."""
    A3, single = _bands(AB)
    Z, n_sets, cols = _rhs_sets(Z, A3.shape[2], n_sets)
    if resolve_backend(backend) == "cpu":
        G, sld, info, L = _cpu_gram(A3, Z, n_sets, cols)
    else:
        G, sld, info, L = _handle(device).gram(A3, Z, n_sets, want_factor=return_factor)
    out = (G[0], float(sld[0]), int(info[0])) if single else (G, sld, info)
    if return_factor:
        out += (L[0] if single else L,)
    return out


def banded_forward(L, Z, device=None, backend=None):
    """``Y = L^-1 Z`` for a factor L in the band layout, ``(b + 1, n)`` or ``(m, b + 1, n)``, and the columns Z ``(n,)`` or
    ``(n, ncols)``: ``(n, ncols)`` or ``(m, n, ncols)``."""
    L3, single = _bands(L, "L")
    Z = np.asarray(Z, dtype=float)
    vec = Z.ndim == 1
    if vec:
        Z = Z[:, None]
    if Z.ndim != 2 or Z.shape[0] != L3.shape[2] or Z.shape[1] < 1:
        raise ValueError(f"Z must have shape ({L3.shape[2]},) or ({L3.shape[2]}, ncols), got {Z.shape}")
    Y = _cpu_forward(L3, Z) if resolve_backend(backend) == "cpu" else _handle(device).forward(L3, Z)
    if vec:
        Y = Y[:, :, 0]
    return Y[0] if single else Y


def gram_of_descs(descs, X, nugget, Z, n_sets, device=None, backend=None):
    """``(G, sum_log_diag, info)`` of the model layer (``structure="banded"``): the bands of the descriptors at the widest member's
    half-bandwidth and their Gram matrices; on the device the bands are built and factorised there and never cross the bus."""
    for d in descs:
        check_monotone(d)
    w = _checked_widths(descs, X, nugget, device, backend)
    if resolve_backend(backend) == "cpu":                  # one matrix at a time at its own width: LAPACK's blocking depends on the width
        parts = [_cpu_gram(_cpu_build([d], X, nugget, int(b)), Z, n_sets, Z.shape[1] // n_sets)[:3] for d, b in zip(descs, w)]
        return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))
    return _handle(device).build_gram(descs, X[:, 0], nugget, int(np.max(w)), np.asarray(Z, dtype=float), n_sets)
