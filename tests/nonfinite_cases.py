"""Inputs and expectations of the non-finite and degenerate-input tests (tests/test_nonfinite_cpu.py, tests/test_gpu_nonfinite.py;
DESIGN.md section 25).  No tests here.

Three kinds of input:

* a point, a right-hand-side entry or an uploaded entry that is NaN, +inf or -inf (``plant_point``, ``plant_rhs``, ``UPPER_PLANTS``);
* a hyperparameter at the end of an optimiser's walk: a length scale of 1e300 or inf (the all-ones matrix), an amplitude of 0,
  a length scale of 0 or NaN (refused by ``describe_kernel``);
* the finite but degenerate kernel ``C(a) RBF(1e-3) + White(w)`` on the 0.1 grid, whose matrix is exactly s I: every likelihood
  piece has a closed form, evaluated here in ``numpy.longdouble`` from the float64 inputs (``closed_form``).

The info reference is ``dpotf2`` below -- netlib's unblocked lower Cholesky with its pivot test ``ajj <= 0 or isnan(ajj)`` -- on
scikit-learn's matrix.  An optimised LAPACK cannot serve: it may leave the NaN half of the test out and return info 0."""
from __future__ import annotations

import functools

import numpy as np
from sklearn.gaussian_process.kernels import RBF, ConstantKernel as C, Matern, WhiteKernel

DX = 0.1
EPS = float(np.finfo(np.float64).eps)
NUGGET = 1e-10
NONFINITE = (np.nan, np.inf, -np.inf)

# orders by route (include/gsum_hip.h: n <= 128 one workgroup; above it k_lml_medium, the grouped schedule or a single factorisation)
ONE_WORKGROUP = (1, 2, 17, 128)
MEDIUM = (129, 257, 385)
LARGE = (641, 1100)                    # np = 768: the persistent chain engages; np = 1280: five panels, macro-steps deeper than one
GRADIENT = (17, 128, 129, 257)
OPERATOR = (129, 641)
OPERATOR_K = (1, 5, 16)
PLANT_ROWS = (0, 1, 15, 16, 127, 128, 255, 256)


def grid(n):
    return DX * np.arange(n, dtype=float)[:, None]


def rhs(n, k=4, seed=7):
    return np.random.RandomState(seed).randn(n, k)


def plant_rows(n):
    """the planted rows that lie inside the order, with the last one"""
    return sorted({i for i in PLANT_ROWS if i < n} | {n - 1})


def plant_point(X, i, value=np.nan):
    X = np.array(X, dtype=float)
    X[i] = value
    return X


def plant_rhs(Z, r, c, value):
    Z = np.array(Z, dtype=float)
    Z[r, c] = value
    return Z


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------
def banded():
    """RBF(0.2) on the 0.1 grid: exp(-12.5 j^2) is 0.0 from lag 78 on -- exact zeros, the grouped schedule's skips are active"""
    return RBF(0.2)


def dense():
    """Matern-3/2 with length scale 5: no entry underflows at any order used here"""
    return Matern(5.0, nu=1.5)


def tree():
    """a Sum of two stationary terms: the device evaluates it entry by entry as a tree (k_build_tree)"""
    return C(1.25) * RBF(0.5) + C(0.75) * Matern(2.0, nu=1.5) + WhiteKernel(0.5)


KERNELS = {"banded": banded, "dense": dense, "tree": tree}


def sk_matrix(kernel, X, nugget=NUGGET):
    """scikit-learn's float64 matrix of the one-argument form, nugget on the diagonal"""
    with np.errstate(all="ignore"):
        K = np.array(kernel(np.asarray(X, dtype=float)))
    K[np.diag_indices_from(K)] += nugget
    return K


def classes(A):
    """entry classes: 0 exact zero, 1 finite nonzero, 2 +inf, 3 -inf, 4 NaN"""
    A = np.asarray(A, dtype=float)
    out = np.ones(A.shape, dtype=np.int8)
    out[A == 0.0] = 0
    out[A == np.inf] = 2
    out[A == -np.inf] = 3
    out[np.isnan(A)] = 4
    return out


# ---- netlib's rule ---------------------------------------------------------------------------------------------------------------------
def dpotf2(A):
    """netlib dpotf2, uplo = 'L', in plain numpy: (L, info).  Column j: ajj = A_jj - L_j,:j . L_j,:j; refused -- info = j + 1, the
    columns before it stay -- when ``ajj <= 0 or isnan(ajj)``; else L_jj = sqrt(ajj) and the column below is scaled.  Reads the lower
    triangle only."""
    A = np.asarray(A, dtype=float)
    n = A.shape[0]
    L = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            row = L[j, :j]
            ajj = A[j, j] - row @ row
            if ajj <= 0.0 or np.isnan(ajj):
                return L, j + 1
            ajj = np.sqrt(ajj)
            L[j, j] = ajj
            if j + 1 < n:
                L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ row) / ajj
    return L, 0


def info_of_nan_point(n, i):
    """First refused pivot when X[i] is NaN: row and column i are NaN off a finite diagonal.  Pivot i >= 1 has NaN products in its sum;
    with i = 0 the first contaminated pivot is 1 (through L_10); a 1 x 1 matrix has no off-diagonal entry."""
    if n == 1:
        return 0
    return i + 1 if i >= 1 else 2


@functools.lru_cache(maxsize=None)
def clean_info(name, n):
    """info of the clean matrix by netlib's rule (0 for every kernel and order used: asserted on the CPU)"""
    return dpotf2(sk_matrix(KERNELS[name](), grid(n)))[1]


# ---- degenerate hyperparameters --------------------------------------------------------------------------------------------------------
def healthy(ls):
    return C(1.0) * RBF(ls) + WhiteKernel(1e-6)


def bad_members():
    """name -> (kernel, info with nugget 0).  White(1e-300) keeps the hyperparameter structure of ``healthy`` (a gradient batch needs
    one structure) and vanishes against the unit diagonal: fl(1 + 1e-300) = 1, the all-ones matrix, pivot 1 = 1 - 1 = 0 exactly."""
    return {
        "ls_1e300": (C(1.0) * RBF(1e300) + WhiteKernel(1e-300), 2),
        "ls_inf": (C(1.0) * RBF(np.inf) + WhiteKernel(1e-300), 2),
        # 0 * K + 0 * I: the zero matrix, pivot 0 refused (fixed: log 0 is no theta)
        "amp_0": (C(0.0, constant_value_bounds="fixed") * RBF(0.3) + WhiteKernel(0.0, noise_level_bounds="fixed"), 1),
    }


GRAD_BAD = ("ls_1e300", "ls_inf")              # the members with the free structure of ``healthy``
REFUSED_LENGTH_SCALES = (0.0, -1.0, np.nan)
BATCHES = (5, 23)
WAVE_SHAPES = ((3, 2), (2, 3))                  # (wave_groups, wave_size): the bad member shares a group, a call takes several rounds


def batch_length_scales(m):
    """m distinct healthy length scales on the 0.1 grid (with White(1e-6): positive definite without a nugget)"""
    return [0.15 + 0.01 * j for j in range(m)]


def bad_positions(m):
    return (0, m // 2, m - 1)


# ---- uplo = 'L' ------------------------------------------------------------------------------------------------------------------------
def upper_plants(n):
    """(row, column) of strict upper-triangle entries: inside the first diagonal 16 x 16 block, inside a diagonal 128 x 128 block but
    outside its 16 x 16 ones, outside every diagonal 128 x 128 block, in the last column"""
    out = [(0, 1), (3, 14), (2, 100), (17, 127)]
    if n > 140:
        out += [(5, 130), (127, 128), (129, 140)]
    out += [(0, n - 1), (n - 2, n - 1)]
    return [(r, c) for r, c in out if r < c < n]


# ---- the closed form -------------------------------------------------------------------------------------------------------------------
CLOSED_A, CLOSED_W = 2.5, 0.75


def closed_kernel(a=CLOSED_A, w=CLOSED_W):
    """C(a) RBF(1e-3) + White(w) on the 0.1 grid: exp(-0.5 (100 j)^2) = 0.0 for every lag j >= 1, the matrix is (a + w) I exactly.
    With a = 0: C(0) RBF(0.2) + White(w), 0 * K_ij = 0 off the diagonal: w I."""
    if a == 0.0:
        return C(0.0, constant_value_bounds="fixed") * RBF(0.2) + WhiteKernel(w)
    return C(a) * RBF(1e-3) + WhiteKernel(w)


def closed_scale(a=CLOSED_A, w=CLOSED_W, nugget=NUGGET):
    """s = fl(fl(fl(a * 1) + w) + nugget): amplitude times the unit diagonal, then the noise, then the nugget -- scikit-learn's
    association (Product, Sum, then the caller's nugget) and the build kernels' (gs_edge_value).  The tests assert it through the
    diagonal that to_host returns."""
    return float(np.float64(np.float64(np.float64(a) * 1.0 + np.float64(w)) + np.float64(nugget)))


def closed_form(Z, a=CLOSED_A, w=CLOSED_W, nugget=NUGGET):
    """Truth in long double from the float64 inputs, and the derived bounds:
        G = Z^T Z / s,  sum log L_ii = (n / 2) log s,  tr(R^-1 dR_amplitude) = n a / s,  tr(R^-1 dR_white) = n w / s,
        tr(R^-1 dR_length) = 0 and H_length = 0 exactly,  H_amplitude = a Z^T Z / s^2,  H_white = w Z^T Z / s^2.
    |G - truth| <= (n + 8) eps |Z|^T |Z| / s: the dot-product bound n eps of a sum of n products in any order, plus the roundings of
    the reciprocal square root, of the two scalings by it and of the sum's last subtraction.  |sld - truth| <= eps (n + 1) |truth| +
    n eps: the sum of n equal terms log L_ii = |truth| / n in any order costs (n - 1) eps |truth|, the rounding of each logarithm
    eps |truth| in all, and an L_ii that is off by a few eps moves its logarithm by as many eps absolutely: the n eps (DESIGN.md
    section 22's form).  Traces:
    (n + 8) eps |truth|.  H_amplitude and H_white: V = R^-1 Z costs four scalings by the reciprocal square root, dR V one more product,
    the contraction a sum of n: (n + 16) eps a |Z|^T |Z| / s^2."""
    ld = np.longdouble
    Z = np.asarray(Z, dtype=float)
    n = Z.shape[0]
    s = ld(closed_scale(a, w, nugget))
    ZtZ = Z.astype(ld).T @ Z.astype(ld)
    absZtZ = np.abs(Z).astype(ld).T @ np.abs(Z).astype(ld)
    G = ZtZ / s
    sld = ld(n) / 2 * np.log(s)
    tr = {"amplitude": ld(n) * ld(a) / s, "white": ld(n) * ld(w) / s, "length": ld(0)}
    H = {"amplitude": ld(a) * ZtZ / (s * s), "white": ld(w) * ZtZ / (s * s), "length": np.zeros_like(ZtZ)}
    bounds = dict(G=(n + 8) * EPS * absZtZ / s, sld=EPS * (n + 1) * abs(sld) + n * EPS,
                  trace={k: (n + 8) * EPS * abs(v) for k, v in tr.items()},
                  H={"amplitude": (n + 16) * EPS * ld(a) * absZtZ / (s * s), "white": (n + 16) * EPS * ld(w) * absZtZ / (s * s),
                     "length": np.zeros_like(ZtZ)})
    return dict(n=n, s=float(s), G=G, sld=sld, trace=tr, H=H, bounds=bounds)


def closed_ratios(cf, G, sld, trace=None, H=None, order=None):
    """achieved / bound of every piece (the largest over a matrix's entries); ``order``: the names of trace's and H's entries.  Where
    the bound is zero the value must be exactly zero: reported as 0.0 or inf."""
    ld = np.longdouble

    def ratio(err, bound):
        err, bound = np.asarray(err, dtype=ld), np.asarray(bound, dtype=ld)
        with np.errstate(all="ignore"):
            r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
        return float(np.max(r)) if r.size else 0.0

    out = dict(G=ratio(np.abs(np.asarray(G).astype(ld) - cf["G"]), cf["bounds"]["G"]),
               sld=ratio(abs(ld(sld) - cf["sld"]), cf["bounds"]["sld"]))
    if trace is not None:
        for p, name in enumerate(order):
            out["trace_" + name] = ratio(abs(ld(trace[p]) - cf["trace"][name]), cf["bounds"]["trace"][name])
            out["H_" + name] = ratio(np.abs(np.asarray(H[p]).astype(ld) - cf["H"][name]), cf["bounds"]["H"][name])
    return out


def gradient_order(kernel):
    """names of kernel.theta's components for ``closed_kernel`` (scikit-learn's order: leaves left to right)"""
    names = []
    for h in kernel.hyperparameters:
        if h.fixed:
            continue
        names.append("amplitude" if "constant_value" in h.name else ("white" if "noise_level" in h.name else "length"))
    return names
