"""Inputs and truths shared by test_loo_cpu.py and test_gpu_loo.py (no tests here).

Exact lattices: factors whose inverse, precision diagonal and solves are small integers, so every sum is exact in fp64 in any
order and the results are compared bit for bit.

    subdiag(n):  L = I + subdiag(1)   W = L^-1 has W_ij = (-1)^(i-j) for i >= j   p_j = n - j
    ones(n):     L = tril(ones)       W = I - subdiag(1)                          p = (2, ..., 2, 1)

Random SPD classes: three kernels on points one spacing apart (or uniform in the unit square), a nugget each.  The truth of a
case is the numpy.longdouble inverse of the SAME float64 factor the code under test gets, so that only the triangular inverse and
its products are judged, not a Cholesky factorisation.
"""
import functools

import numpy as np

# one block, two blocks, an odd block count, unequal halves at two levels of the merge (blocks of 128)
LATTICE_SIZES = (1, 2, 127, 128, 129, 255, 256, 257, 383, 384, 385, 640, 641)
RANDOM_SIZES = (129, 257, 641)
FLOOR = 64 * 2.0 ** -53
COND_LIMIT = 1e6


def lattice(kind, n):
    """(L, W, p) of an exact lattice, W and p as int64."""
    if kind == "subdiag":
        L = np.eye(n) + np.eye(n, k=-1)
        i, j = np.indices((n, n))
        W = np.where(i >= j, 1 - 2 * ((i - j) % 2), 0).astype(np.int64)
        p = n - np.arange(n, dtype=np.int64)
    elif kind == "ones":
        L = np.tril(np.ones((n, n)))
        W = (np.eye(n) - np.eye(n, k=-1)).astype(np.int64)
        p = np.full(n, 2, dtype=np.int64)
        p[-1] = 1
    else:
        raise ValueError(kind)
    return L, W, p


def integer_rhs(n, k, seed=0):
    """Integers in [-3, 3]: W^T (W R) of a lattice stays far below 2^53."""
    return np.random.RandomState(seed).randint(-3, 4, size=(n, k)).astype(float)


def lattice_alpha(W, R):
    """(L L^T)^-1 R of a lattice, exactly (int64 arithmetic)."""
    return (W.T @ (W @ R.astype(np.int64))).astype(float)


# -- random SPD classes ------------------------------------------------------------------------------------------------
# name -> (kernel matrix without nugget, nugget).  'rbf_l2' is the RBF at a length scale of two spacings; its condition number,
# 4.9e6 at every size here, is above COND_LIMIT, so the class whose condition number is 8 ('rbf': three quarters of a spacing)
# runs beside it and the limit is asserted for the classes in CONDITIONED.
def _grid_sqdist(n):
    x = np.arange(n, dtype=float)
    return (x[:, None] - x[None, :]) ** 2


def _rbf(n, ell):
    return np.exp(-0.5 * _grid_sqdist(n) / ell ** 2)


def _matern52(n, ell):
    s = np.sqrt(5.0) * np.sqrt(_grid_sqdist(n)) / ell
    return (1 + s + s * s / 3) * np.exp(-s)


def _rbf2d(n, ell):
    X = np.random.RandomState(0).rand(n, 2)
    return np.exp(-0.5 * ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1) / ell ** 2)


CLASSES = {
    "rbf_l2": (lambda n: _rbf(n, 2.0), 1e-6),
    "rbf": (lambda n: _rbf(n, 0.75), 1e-6),
    "matern52": (lambda n: _matern52(n, 4.0), 1e-8),
    "rbf2d": (lambda n: _rbf2d(n, 0.15), 1e-4),
}
CONDITIONED = ("rbf", "matern52", "rbf2d")


@functools.lru_cache(maxsize=None)
def spd(name, n):
    """The covariance of a class at size n (read-only)."""
    base, nugget = CLASSES[name]
    K = base(n) + nugget * np.eye(n)
    K.setflags(write=False)
    return K


def curves(n, k, seed=1):
    return np.random.RandomState(seed).standard_normal((n, k))


def tri_inverse_ld(L):
    """L^-1 of a lower-triangular L in numpy.longdouble, by forward substitution, row by row."""
    L = np.tril(np.asarray(L)).astype(np.longdouble)
    n = L.shape[0]
    W = np.zeros((n, n), dtype=np.longdouble)
    for i in range(n):
        W[i, :i] = -(L[i, :i] @ W[:i, :i]) / L[i, i]
        W[i, i] = 1 / L[i, i]
    return W


def cholesky_ld(K):
    """The lower Cholesky factor of K in numpy.longdouble."""
    K = np.asarray(K).astype(np.longdouble)
    n = K.shape[0]
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def truth_from_factor_ld(L, R):
    """(p, alpha) of (L L^T)^-1 in long double from a factor L (float64 or long double) and residuals R (n, k)."""
    W = tri_inverse_ld(L)
    return (W * W).sum(0), W.T @ (W @ R.astype(np.longdouble))


@functools.lru_cache(maxsize=None)
def factor_case(name, n, k=3):
    """(L, R, p_truth, alpha_truth): numpy's float64 factor of the class, k residual curves and the long-double truth from that L."""
    L = np.linalg.cholesky(spd(name, n))
    R = curves(n, k)
    p, a = truth_from_factor_ld(L, R)
    for arr in (L, R, p, a):
        arr.setflags(write=False)
    return L, R, p, a


def rel_p(p, truth):
    return float(np.max(np.abs(p.astype(np.longdouble) - truth) / truth))


def rel_a(a, truth):
    return float(np.max(np.abs(a.astype(np.longdouble) - truth)) / np.max(np.abs(truth)))
