"""Leave-one-out diagnostics of N(mean, K) from one Cholesky factor K = L L^T (Rasmussen & Williams 5.4.2).

With r = y - mean, a = K^-1 r and p = diag(K^-1), the prediction of point i from all the others is closed-form:

    loo_mean_i   = y_i - a_i / p_i
    loo_var_i    = 1 / p_i
    loo_error_i  = a_i / sqrt(p_i)                               (standardised: N(0, 1) under the model)
    loo_logpdf_i = -1/2 log 2 pi + 1/2 log p_i - 1/2 a_i^2 / p_i

p needs W = L^-1 (p_j = sum_i W_ij^2), the only O(n^3) piece.  On ``backend='hip'`` libgsum_loo.so (include/gsum_loo.h, DESIGN.md
section 15) forms W on the device and keeps it there; ``backend='cpu'`` is the same arithmetic on scipy's ``solve_triangular``.
``Diagnostic.loo`` and ``ConjugateGaussianProcess.loo`` are built on ``LooFactor``.

Leave-group-out (k-fold, leave-a-block-out, leave-every-third-point-out) is closed-form from the same W.  With P = K^-1 = W^T W,
the points of a group G are predicted from the points outside it by

    y_G - E[y_G | y_-G] = P_GG^-1 a_G          Cov[y_G | y_-G] = P_GG^-1

and with P_GG = C C^T, V = C^-1 and z = V a_G: the residual is V^T z, the marginal variances are the column sums of squares of V,
md2 = z^T z is the group's squared Mahalanobis distance under its predictive distribution, log det Cov = -2 sum_i log C_ii and
logpdf = -1/2 md2 - 1/2 log det Cov - g/2 log 2 pi.  A group of one point is the leave-one-out above.  On 'hip' log det Cov also
carries the first-order correction tr(V P_GG V^T) - g, taken from the gathered columns of W.  ``LooFactor.folds``,
``kfold_from_factor``, ``Diagnostic.kfold`` and ``ConjugateGaussianProcess.kfold``.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from ._backend import resolve_backend, resolve_device

__all__ = ["LooResult", "FoldResult", "LooFactor", "loo_from_factor", "kfold_from_factor", "make_folds"]

LooResult = namedtuple("LooResult", ["mean", "var", "error", "logpdf", "precision_diag"])
LooResult.__doc__ = """The leave-one-out predictions of every point: ``mean``, ``error`` and ``logpdf`` have y's shape, (n,) or
(n, n_curves); ``var`` and ``precision_diag`` (p = diag(K^-1) = 1 / var) are (n,), the same for every curve."""

FoldResult = namedtuple("FoldResult", ["mean", "var", "error", "md2", "logpdf", "fold_of"])
FoldResult.__doc__ = """The leave-group-out predictions of every point from the points outside its group: ``mean`` and ``error``
(the residual over the square root of ``var``) have y's shape; ``var`` (the marginal predictive variance) and ``fold_of`` (each
point's group number) are (n,); ``md2`` (the squared Mahalanobis distance of a group under its joint predictive distribution) and
``logpdf`` (its log density) are (n_folds,) or (n_folds, n_curves)."""


def make_folds(n, k, kind="blocks", random_state=None):
    """A label array (n,) of k groups: 'blocks' (contiguous, the sizes of ``numpy.array_split``), 'interleaved' (point i in group
    i mod k) or 'random' (a random permutation cut into the blocks' sizes; ``random_state`` a seed or a RandomState)."""
    n, k = int(n), int(k)
    if n < 1 or not 1 <= k <= n:
        raise ValueError(f"make_folds needs 1 <= k <= n, got n = {n}, k = {k}")
    blocks = np.repeat(np.arange(k), [len(a) for a in np.array_split(np.arange(n), k)])
    if kind == "blocks":
        return blocks
    if kind == "interleaved":
        return np.arange(n) % k
    if kind == "random":
        rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
        labels = np.empty(n, dtype=blocks.dtype)
        labels[rs.permutation(n)] = blocks
        return labels
    raise ValueError(f"kind must be 'blocks', 'interleaved' or 'random', got {kind!r}")


def _as_index_array(a, what):
    a = np.asarray(a)
    if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be a non-empty one-dimensional integer array, got shape {a.shape}, dtype {a.dtype}")
    return a.astype(np.int64)


def normalise_folds(folds, n):
    """(fold_ptr (n_folds + 1,), fold_idx (n,), fold_of (n,)) of ``folds``: an integer k (k contiguous blocks), a label array (n,)
    of integers (groups numbered by ascending label) or a sequence of index arrays that partition 0 .. n - 1.  ValueError for
    anything else."""
    if isinstance(folds, (bool, np.bool_)):
        raise ValueError("folds must be an integer, a label array or a sequence of index arrays, got a bool")
    if isinstance(folds, (int, np.integer)):
        if not 1 <= folds <= n:
            raise ValueError(f"the number of folds must be in 1 ... {n}, got {folds}")
        folds = make_folds(n, int(folds))
    try:
        arr = np.asarray(folds)
    except ValueError:                                              # ragged: a sequence of index arrays
        arr = None
    if arr is not None and arr.dtype != object and arr.ndim == 1:
        if arr.dtype.kind not in "iu" or arr.shape != (n,):
            raise ValueError(f"a label array must be ({n},) of integers, got shape {arr.shape}, dtype {arr.dtype}")
        _, fold_of = np.unique(arr, return_inverse=True)
        fold_of = fold_of.reshape(-1).astype(np.int64)
        fold_idx = np.argsort(fold_of, kind="stable").astype(np.int64)
        fold_ptr = np.concatenate([[0], np.cumsum(np.bincount(fold_of))]).astype(np.int64)
        return fold_ptr, fold_idx, fold_of
    try:
        groups = [_as_index_array(g, f"group {q}") for q, g in enumerate(folds)]
    except TypeError:
        raise ValueError("folds must be an integer, a label array or a sequence of index arrays") from None
    if not groups:
        raise ValueError("folds holds no group")
    fold_idx = np.concatenate(groups)
    if fold_idx.size != n or fold_idx.min() < 0 or fold_idx.max() >= n or np.any(np.bincount(fold_idx, minlength=n) != 1):
        raise ValueError(f"the groups must partition 0 ... {n - 1}: every point in exactly one group")
    fold_ptr = np.concatenate([[0], np.cumsum([g.size for g in groups])]).astype(np.int64)
    fold_of = np.empty(n, dtype=np.int64)
    fold_of[fold_idx] = np.repeat(np.arange(len(groups)), [g.size for g in groups])
    return fold_ptr, fold_idx, fold_of


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

    def precision_block(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        if idx.ndim != 1 or idx.size < 1 or idx.min() < 0 or idx.max() >= self.n or np.unique(idx).size != idx.size:
            raise ValueError(f"idx must hold distinct indices in 0 ... {self.n - 1}")
        Wg = self._W[:, idx]
        return Wg.T @ Wg

    def folds(self, fold_ptr, fold_idx, R):
        """The five steps of the module's docstring, group by group and curve by curve (so that neither depends on the others)."""
        from scipy.linalg import solve_triangular
        n, k, nf = self.n, R.shape[1], len(fold_ptr) - 1
        a = np.stack([self._W.T @ (self._W @ R[:, j]) for j in range(k)], axis=1)
        resid, var, md2, logdet = np.empty((n, k)), np.empty(n), np.empty((nf, k)), np.empty(nf)
        for q in range(nf):
            G = np.sort(fold_idx[fold_ptr[q]:fold_ptr[q + 1]])
            Wg = self._W[G[0]:, G]                                  # column j of W is zero above row j
            P = Wg.T @ Wg
            try:
                if not np.all(np.isfinite(P)):
                    raise np.linalg.LinAlgError("not finite")
                C = np.linalg.cholesky(P)
                if not np.all(np.isfinite(C)) or not np.all(np.diag(C) > 0):
                    raise np.linalg.LinAlgError("not positive definite")
            except np.linalg.LinAlgError:
                raise np.linalg.LinAlgError(f"group {q} does not factor: its block of the precision matrix is not positive definite") from None
            V = solve_triangular(C, np.eye(G.size), lower=True)
            for j in range(k):
                z = V @ a[G, j]
                resid[G, j] = V.T @ z
                md2[q, j] = z @ z
            var[G] = (V * V).sum(0)
            logdet[q] = -2.0 * np.sum(np.log(np.diag(C)))
        return resid, var, md2, logdet

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
        self.fold_budget = None                     # 'hip': the bytes one chunk of groups may take in folds (None: what is free)

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

    def precision_block(self, idx):
        """The rows and columns ``idx`` (distinct, any order) of K^-1 = (L L^T)^-1, shape (g, g), in the order of ``idx``."""
        idx = np.asarray(idx)
        if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in "iu":
            raise ValueError(f"idx must be a non-empty one-dimensional integer array, got shape {idx.shape}, dtype {idx.dtype}")
        return self._f.precision_block(idx.astype(np.int64))

    def folds(self, y, folds, mean=0.0):
        """``FoldResult`` of the curves y, (n,) or (n, n_curves), under N(mean, L L^T): every point predicted from the points outside
        its group.  ``folds``: an integer k (k contiguous blocks with the sizes of ``numpy.array_split``), a label array (n,) of
        integers (groups numbered by ascending label; ``make_folds``) or a sequence of index arrays that partition the points.
        ValueError for anything else; numpy.linalg.LinAlgError, naming the group, where a group's block of K^-1 does not factor."""
        y = np.asarray(y, dtype=float)
        if y.ndim not in (1, 2) or y.shape[0] != self.n or y.size == 0:
            raise ValueError(f"y must be ({self.n},) or ({self.n}, n_curves), got {y.shape}")
        mean = np.asarray(mean, dtype=float)
        if mean.shape not in ((), (self.n,)):
            raise ValueError(f"mean must be a scalar or ({self.n},), got {mean.shape}")
        r = (y.T - mean).T.reshape(self.n, -1)
        fold_ptr, fold_of, (resid, var, md2, logdet) = self._raw_folds(folds, r)
        sizes = np.diff(fold_ptr).astype(float)
        logpdf = -0.5 * md2 - 0.5 * logdet[:, None] - 0.5 * sizes[:, None] * np.log(2 * np.pi)
        error = resid / np.sqrt(var)[:, None]
        if y.ndim == 1:
            resid, error, md2, logpdf = resid[:, 0], error[:, 0], md2[:, 0], logpdf[:, 0]
        return FoldResult(mean=y - resid, var=var, error=error, md2=md2, logpdf=logpdf, fold_of=fold_of)

    def _raw_folds(self, folds, r):
        """(fold_ptr, fold_of, (resid (n, k), var (n,), md2 (n_folds, k), logdet (n_folds,))) of the residual curves r (n, k): what
        the backend computes, before ``folds`` turns it into a ``FoldResult``."""
        fold_ptr, fold_idx, fold_of = normalise_folds(folds, self.n)
        if self.backend != "cpu":
            self._f.set_fold_budget(self.fold_budget or 0)
        return fold_ptr, fold_of, self._f.folds(fold_ptr, fold_idx, np.ascontiguousarray(r, dtype=float))

    def times(self, reset=False):
        """Device milliseconds by phase (``_loo_lib.PHASES``); 'hip' only."""
        return self._f.times(reset)

    def fold_times(self, reset=False):
        """Device milliseconds of ``folds`` and ``precision_block`` by phase (``_loo_lib.FOLD_PHASES``); 'hip' only."""
        return self._f.fold_times(reset)

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


def kfold_from_factor(L, y, folds, mean=0.0, device=None, backend=None):
    """``FoldResult`` of y, (n,) or (n, n_curves), under N(mean, L L^T) from the lower Cholesky factor L alone (``LooFactor.folds``)."""
    f = LooFactor(L, device=device, backend=backend)
    try:
        return f.folds(y, folds, mean)
    finally:
        f.free()
