"""Inputs of the zero-skip tests (tests/test_zero_skip_cpu.py, tests/test_gpu_zero_skip.py): kernel matrices whose Cholesky factors have
exactly-zero blocks of every shape the grouped batch schedule's flags and K windows meet, plus dense ones.  Seeded; n = 1296 pads to
np = 1536 (six outer steps of 256 columns) unless noted.  Every case carries 3 to 6 kernels; the structural claim is about the first."""
from __future__ import annotations

import functools

import numpy as np
from sklearn.gaussian_process.kernels import RBF, Matern

N = 1296
DX = 0.1


def grid(n=N):
    return DX * np.arange(n)[:, None]


def rhs(n, seed, zero_column=None):
    """k = 4: three random columns and the column of ones (the constant basis function)."""
    Z = np.concatenate([np.random.RandomState(seed).randn(n, 3), np.ones((n, 1))], axis=1)
    if zero_column is not None:
        Z[:, zero_column] = 0.0
    return Z


def clusters(block, n=N):
    """Two clusters 1000 apart, interleaved by index in blocks of `block` points; each cluster's points are consecutive in position."""
    which = (np.arange(n) // block) % 2
    pos = np.empty(n)
    for c in (0, 1):
        idx = np.flatnonzero(which == c)
        pos[idx] = 1000.0 * c + DX * np.arange(idx.size)
    return pos[:, None]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(X, Z, nugget, kernels, halfwidth | None, dense, holes)"""
    out = {}

    def add(name, X, kernels, nugget=1e-10, halfwidth=None, dense=False, holes=False, zero_column=None):
        out[name] = dict(X=X, Z=rhs(X.shape[0], len(out) + 1, zero_column), nugget=nugget, kernels=kernels, halfwidth=halfwidth, dense=dense,
                         holes=holes)

    # (a) the band of 77 lies inside one tile row; lags 76 and 77 are subnormal
    add("a", grid(), [RBF(0.2), RBF(0.19), RBF(0.195), RBF(0.2)], halfwidth=77)
    # The nugget of (b), (c) and (d) is 1e-6.  At ell >= 0.35 the smallest eigenvalue of the RBF matrix at dx = 0.1 lies below 1e-25, so the
    # nugget IS the smallest eigenvalue and the condition number is ~10 / nugget.  With 1e-10 (condition 1e11) the CPU reference itself is
    # not defined to 1e-10: two fp64 factorisations that only sum in different orders (scipy's and the blocked numpy model of
    # test_zero_skip_cpu.py) give log-likelihoods 5e-10 ... 1e-8 apart on these matrices, for white-noise and for GP-drawn right-hand sides
    # alike -- no fp64 code can be held to 1e-10 of either.  With 1e-6 (condition 1e7, below the 2e8 of the S-type input on which the
    # project's 1e-10 bar is stated) they agree to 1e-12, which test_zero_skip_cpu.py asserts for every case.  The
    # band widths do not depend on the nugget.
    # (b) the band of 135 crosses a 128 boundary
    add("b", grid(), [RBF(0.35), RBF(0.33), RBF(0.3)], nugget=1e-6, halfwidth=135)
    # (c) the band of 193 reaches into the sibling block
    add("c", grid(), [RBF(0.5), RBF(0.45), RBF(0.4)], nugget=1e-6, halfwidth=193)
    # (d) the band of 347 is wider than a panel
    add("d", grid(), [RBF(0.9), RBF(0.8), RBF(0.7)], nugget=1e-6, halfwidth=347)
    # (e) dense: length scales at which no entry of the matrix or of its factor underflows (exp(-sqrt(5) r / ell) is 0.0 from r = 333 ell on),
    # and n = np = 1536 -- the padding rows of any other order are exactly zero under every panel, and their tiles are skipped
    add("e", grid(1536), [Matern(1.0, nu=2.5), Matern(0.8, nu=2.5), Matern(1.2, nu=2.5)], dense=True)
    # (f) two interleaved clusters: zero row groups between nonzero ones.  A row couples to the 7 points before it in ITS cluster
    # (ell = 0.02: exp(-12.5 k^2) is 0.0 from k = 8 on), so under a panel that ends inside a block the rest of the block is nonzero for 7
    # rows, then zero, and the next block of the same cluster further down is zero throughout while the other cluster's block between
    # them starts nonzero again.  (With ell = 0.2 both clusters reach 77 points back, across every block of 40 or 48: the second kernel.)
    for block in (40, 48, 272):
        add(f"f{block}", clusters(block), [RBF(0.02), RBF(0.2), RBF(0.021)], holes=True)
    # (g) the smallest orders with deep macro-steps: np = 1024 and 1280
    add("g1024", grid(1024), [RBF(0.2), RBF(0.19), RBF(0.195)])
    add("g1040", grid(1040), [RBF(0.2), RBF(0.19), RBF(0.195)])
    # (h) one right-hand-side column all zero
    add("h", grid(), [RBF(0.2), RBF(0.195), RBF(0.19)], zero_column=1)
    return out


def kernel_matrix(case, i=0):
    K = case["kernels"][i](case["X"])
    K[np.diag_indices_from(K)] += case["nugget"]
    return K
