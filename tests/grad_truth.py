"""Extended-precision truth for the gradient pieces of gsum_lml_grad[_batch], their error scales and the case matrix (no tests here).

The device returns, per log-hyperparameter p of R = kernel(X) + nugget I:  trace_p = tr(R^-1 dR_p)  and  H_p = V^T dR_p V,  V = R^-1 Z,
beside G = Z^T R^-1 Z and sld = sum_i log L_ii.  ``pieces_truth`` evaluates all of them in ``numpy.longdouble`` (x87: 64-bit mantissa)
from the float64 arrays  R = kern(X) + nugget I  and  dR = kern(X, eval_gradient=True)[1]  taken as EXACT inputs: ``describe_gradient``
documents that device parameter p means exactly ``K_gradient[:, :, p]``.  Cholesky column by column, L^-1 by forward substitution,
R^-1 = L^-T L^-1, then the contractions; nothing compiled, nothing read from a file.

Error scales (free of the conditioning; the conditioning enters once, as cond_2(R)):
    S_trace[p]   = sum_ij |R^-1_ij| |dR_p,ij|
    S_H[p]       = |V|^T |dR_p| |V|                entrywise
    S_G          = |Z|^T |R^-1| |Z|                entrywise
    S_sld        = n max_i |log L_ii|
and the normalised error of a computed piece x is   e(x) = max over its components of |x - truth| / (cond_2(R) S)   (``normalised_error``).

The entrywise S_H is an error scale only where V is dense.  A computed V carries  |dV| <= c eps |R^-1| |R| |V|,  which cond_2(R) |V| bounds
in norm but not entry by entry: with the selector right-hand sides Z = R[:, cols] (V = e_cols up to rounding) an entry of H_p whose
dR_p[cols_a, cols_b] is zero -- every diagonal entry of a length-scale parameter -- has S_H ~ 1e-19 while ANY float64 solve leaves
eps cond |dR_p[:, cols_b]| there (scipy's cho_solve: 1e17 eps under the entrywise scale, tests/test_grad_pieces_cpu.py prints it).  The
selector therefore uses the norm form of the same scale, its Cauchy-Schwarz bound
    S_H_norm[p][a, b] = max(|V_a|_2 | |dR_p| |V_b| |_2,  | |dR_p| |V_a| |_2 |V_b|_2)  >=  S_H[p][a, b],
which for V = e_cols is the 2-norm of column cols_b (or cols_a) of dR_p: an entry of K_gradient is pinned relative to its own column.
"""
from __future__ import annotations

import warnings
import zlib
from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
NUGGET = 1e-10
WHITE_TIGHT, WHITE_AMPLIFIED = 0.5, 1e-6          # every shape runs with both: cond < 1e3, and the rounding-amplified run
BOUND = 16.0                                      # e_dev <= BOUND * max(e_ref, eps)
REF_LIMIT = 4.0                                   # a case whose float64 reference has e_ref > REF_LIMIT * eps gets other inputs


def _require_extended():
    if np.finfo(LD).nmant < 63:
        raise RuntimeError(f"numpy.longdouble has a {np.finfo(LD).nmant}-bit mantissa here: the truth needs at least 63 (x87 extended)")


@dataclass
class Truth:
    cond: float
    sld: float
    trace: np.ndarray       # (P,)
    S_trace: np.ndarray
    S_sld: float
    Rinv: np.ndarray        # (n, n) longdouble
    L: np.ndarray
    dR: np.ndarray          # (n, n, P) longdouble
    rhs: dict = field(default_factory=dict)


@dataclass
class RhsTruth:
    G: np.ndarray           # (k, k)
    H: np.ndarray           # (P, k, k)
    S_G: np.ndarray
    S_H: np.ndarray         # entrywise
    S_H_norm: np.ndarray    # norm form (selector right-hand sides)


def cholesky_ld(R):
    """Lower Cholesky factor of R in long double, column by column."""
    A = np.asarray(R, dtype=LD)
    n = len(A)
    L = np.zeros((n, n), LD)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError(f"leading minor {j + 1} is not positive definite")
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def inverse_lower_ld(L):
    """L^-1 by forward substitution on the identity, row by row."""
    n = len(L)
    Li = np.zeros((n, n), LD)
    for i in range(n):
        Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
        Li[i, i] = 1 / L[i, i]
    return Li


def pieces_truth(R, dR):
    """Everything that does not depend on the right-hand sides; ``add_rhs`` adds G and H_p for a Z."""
    _require_extended()
    R = np.asarray(R, dtype=np.float64)
    dR = np.asarray(dR, dtype=np.float64)
    n = len(R)
    assert R.shape == (n, n) and dR.shape[:2] == (n, n)
    L = cholesky_ld(R)
    Li = inverse_lower_ld(L)
    Rinv = Li.T @ Li
    d = dR.astype(LD)
    logd = np.log(np.diag(L))
    trace = np.einsum("ij,ijp->p", Rinv, d)
    S_trace = np.einsum("ij,ijp->p", np.abs(Rinv), np.abs(d))
    return Truth(cond=float(np.linalg.cond(R)), sld=logd.sum(), trace=trace, S_trace=S_trace,
                 S_sld=n * np.abs(logd).max(), Rinv=Rinv, L=L, dR=d)


def add_rhs(truth: Truth, name, Z):
    Z = np.asarray(Z, dtype=np.float64).astype(LD)
    V = truth.Rinv @ Z
    aV, aZ = np.abs(V), np.abs(Z)
    P, k = truth.dR.shape[2], Z.shape[1]
    H, S_H, S_Hn = np.zeros((P, k, k), LD), np.zeros((P, k, k), LD), np.zeros((P, k, k), LD)
    vn = np.sqrt((V * V).sum(axis=0))
    for p in range(P):
        dp = truth.dR[:, :, p]
        ap = np.abs(dp)
        H[p] = V.T @ (dp @ V)
        aq = ap @ aV
        S_H[p] = aV.T @ aq
        qn = np.sqrt((aq * aq).sum(axis=0))
        S_Hn[p] = np.maximum(np.outer(vn, qn), np.outer(qn, vn))
    truth.rhs[name] = RhsTruth(G=Z.T @ V, H=H, S_G=aZ.T @ (np.abs(truth.Rinv) @ aZ), S_H=S_H, S_H_norm=S_Hn)
    return truth.rhs[name]


def normalised_error(x, truth, cond, S):
    """max over the components of |x - truth| / (cond S), as a float.  A component whose scale is exactly zero (a length-scale parameter at
    n = 1: dR_p = 0) must be exact: 0 if it is, inf if not."""
    err = np.abs(np.asarray(x, dtype=LD) - np.asarray(truth, dtype=LD))
    S = np.broadcast_to(np.asarray(S, dtype=LD), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(S > 0, err / (LD(cond) * S), np.where(err == 0, LD(0), LD(np.inf)))
    if not np.all(np.isfinite(np.asarray(x, dtype=float))):
        return float("inf")
    return float(np.max(e)) if e.size else 0.0


def piece_errors(T: Truth, name, G, sld, trace, H, selector=None):
    """Normalised errors of one evaluation's four pieces for right-hand sides ``name``: dict trace / H / G / sld."""
    r = T.rhs[name]
    selector = name == "selector" if selector is None else selector
    return dict(trace=normalised_error(trace, T.trace, T.cond, T.S_trace),
                H=normalised_error(H, r.H, T.cond, r.S_H_norm if selector else r.S_H),
                G=normalised_error(G, r.G, T.cond, r.S_G),
                sld=normalised_error(sld, T.sld, T.cond, T.S_sld))


def reference_pieces(R, dR, Z):
    """The plain float64 evaluation: numpy.linalg.cholesky, cho_solve, einsum."""
    from scipy.linalg import cho_solve
    L = np.linalg.cholesky(R)
    Rinv = cho_solve((L, True), np.eye(len(R)))
    V = cho_solve((L, True), Z)
    return (Z.T @ V, float(np.log(np.diag(L)).sum()), np.einsum("ij,ijp->p", Rinv, dR), np.einsum("ia,ijp,jb->pab", V, dR, V))


# ---- the case matrix ----------------------------------------------------------------------------------------------------------------
def _kernels():
    from sklearn.gaussian_process.kernels import (RBF, DotProduct, Exponentiation, ExpSineSquared, Matern, RationalQuadratic, WhiteKernel,
                                                  ConstantKernel as C)
    return dict(RBF=RBF, Matern=Matern, W=WhiteKernel, C=C, RQ=RationalQuadratic, ESS=ExpSineSquared, Pow=Exponentiation, Dot=DotProduct, np=np)


@dataclass(frozen=True)
class Case:
    """One shape of the matrix.  ``expr``: the kernel over the names of ``_kernels`` with WHITE standing for the white-noise level of the
    run; ``dup``: rows 0 and n // 2 (and row n - 1 where n > 2) of X coincide pairwise -- the den == 0 branch of Matern-1/2; ``grid``: X is
    the uniform grid ``grid * arange(n)`` (d = 1) instead of random points -- wide enough in length scales that most exp arguments of
    K_gradient lie in the subnormal band or beyond it (tests/build_classes.py)."""
    path: str               # small_flat | small_tree | general_flat | general_tree | general_wide
    n: int
    d: int
    k: int
    expr: str
    dup: bool = False
    side: float = 0.0       # X is uniform on [0, side]^d; 0: 3 + 0.02 n for d = 1, 2.5 otherwise
    grid: float = 0.0       # > 0: X = grid * arange(n)

    @property
    def id(self):
        return f"{self.path}-n{self.n}-d{self.d}-k{self.k}"

    def kernel(self, white):
        ns = _kernels()
        ns["WHITE"] = white
        return eval(self.expr, {"__builtins__": {}}, ns)

    def inputs(self):
        """X, Z_random = [randn(n, k - 1) | 1] and the selector's columns."""
        rng = np.random.RandomState(zlib.crc32(self.id.encode()) & 0x7FFFFFFF)
        n, d, k = self.n, self.d, self.k
        side = self.side or ((3.0 + 0.02 * n) if d == 1 else 2.5)
        X = rng.rand(n, d) * side
        if self.grid:
            assert d == 1 and not self.dup
            X = self.grid * np.arange(n, dtype=float)[:, None]
        pairs = []
        if self.dup and n >= 2:
            X[n // 2] = X[0]
            pairs = [0, n // 2]
            if n > 4:
                X[n - 1] = X[n // 3]
                pairs += [n - 1, n // 3]
        Z = np.concatenate([rng.randn(n, k - 1), np.ones((n, 1))], axis=1)
        # the selector's columns, in this order of priority as far as k reaches: the last row (the half-empty wave of an odd n), row 0, the
        # coincident rows, one column TWICE (H_p[a, b], a != b, then reads the DIAGONAL entry dR_p[c, c]), an adjacent pair, random rows
        want = [n - 1, 0] + pairs + [n // 2 + 1, n // 2 + 1, n // 2 + 2, 63, 64, 127, 128, 255, 256]
        cols = []
        for c in want:
            if 0 <= c < n and len(cols) < k and (c not in cols or (c == n // 2 + 1 and cols.count(c) < 2)):
                cols.append(c)
        while len(cols) < k:
            cols.append(int(rng.randint(n)))
        return X, Z, np.array(cols[:k])

    def matrices(self, white):
        """kernel, X, R = kern(X) + nugget I, dR = K_gradient (float64; Matern-1/2 at coincident points: scikit-learn's own 0 / 0 -> 0)."""
        kern = self.kernel(white)
        X, Z, cols = self.inputs()
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            K, dK = kern(X, eval_gradient=True)
        R = K + NUGGET * np.eye(self.n)
        return kern, X, R, dK, Z, cols


_AMP = "C(1.3) * "
_FOUR = ("C(1.2) * RBF(0.9) + C(0.4) * Matern(1.7, nu=1.5) + C(0.8) * Matern(0.6, nu=2.5) + C(0.3) * RQ(length_scale=1.1, alpha=0.8)"
         " + W(WHITE)")           # the 17-operation four-leaf sum of test_four_scaled_leaves_and_white_noise
_LS8 = "np.array([0.9, 1.4, 1.1, 1.8, 1.2, 2.1, 1.0, 1.6])"

CASES = [
    # ---- one workgroup (k_grad_small<false>), d = 1: n16 rounding on both sides of every multiple of 16 that matters, one to 128 points
    Case("small_flat", 1, 1, 1, "C(1.3) * RBF(0.7) + W(WHITE)"),
    Case("small_flat", 2, 1, 5, "Matern(0.7, nu=2.5) + W(WHITE, noise_level_bounds='fixed')"),
    Case("small_flat", 15, 1, 16, "C(1.3) * Matern(0.7, nu=1.5) + W(WHITE) + C(0.2)"),
    Case("small_flat", 16, 1, 5, "C(0.8) * Matern(0.9, nu=0.5) + W(WHITE, noise_level_bounds='fixed')", dup=True),
    Case("small_flat", 17, 1, 5, "C(1.3) * RBF(0.7) + W(WHITE) + C(0.2)"),
    Case("small_flat", 63, 1, 1, "Matern(0.7, nu=1.5) + W(WHITE)"),
    Case("small_flat", 64, 1, 16, "C(1.3) * Matern(0.7, nu=2.5) + W(WHITE, noise_level_bounds='fixed') + C(0.2)"),
    Case("small_flat", 65, 1, 5, "C(0.8) * Matern(0.9, nu=0.5) + W(WHITE)", dup=True),
    Case("small_flat", 127, 1, 16, "C(1.3) * RBF(0.7) + W(WHITE)"),
    Case("small_flat", 128, 1, 5, "C(1.3) * Matern(0.7, nu=2.5) + W(WHITE) + C(0.2)"),
    # ---- the same kernel, d = 2 and d = GSUM_MAX_D = 8 (anisotropic: one parameter per dimension, eleven parameters at d = 8)
    Case("small_flat", 17, 2, 5, "C(1.3) * Matern([0.7, 1.1], nu=2.5) + W(WHITE)"),
    Case("small_flat", 17, 8, 16, f"C(1.3) * RBF({_LS8}) + W(WHITE) + C(0.2)"),
    Case("small_flat", 128, 2, 5, "C(0.8) * Matern([0.9, 1.4], nu=0.5) + W(WHITE, noise_level_bounds='fixed')", dup=True),
    Case("small_flat", 128, 8, 16, f"C(1.3) * Matern({_LS8}, nu=1.5) + W(WHITE)"),
    # ---- one workgroup, kernel trees (k_grad_small<true>)
    Case("small_tree", 1, 1, 5, "C(0.9) * RBF(0.8) + C(0.4) * RQ(length_scale=1.3, alpha=0.8) + W(WHITE)"),
    Case("small_tree", 17, 1, 5, _FOUR),
    Case("small_tree", 64, 1, 16, "C(1.2) * ESS(length_scale=1.1, periodicity=3.0) * RBF(4.0) + W(WHITE)"),
    Case("small_tree", 128, 2, 5, "RQ(length_scale=1.1, alpha=0.7) * RBF([0.9, 1.7]) + C(0.3) + W(WHITE)"),
    # ---- the general path: k_grad_contract<false, 2> (two rows per wave: every odd n leaves the last wave half empty), split + k_grad_trace
    Case("general_flat", 129, 1, 5, "C(1.3) * RBF(0.7) + W(WHITE)"),
    Case("general_flat", 255, 3, 16, "C(1.3) * Matern([0.7, 1.1, 0.5], nu=2.5) + W(WHITE) + C(0.2)"),
    Case("general_flat", 256, 1, 1, "C(1.3) * Matern(0.7, nu=1.5) + W(WHITE, noise_level_bounds='fixed')"),
    Case("general_flat", 257, 2, 5, "C(0.8) * Matern([0.9, 1.4], nu=0.5) + W(WHITE)", dup=True),
    Case("general_flat", 383, 2, 5, "Matern(0.8, nu=2.5) + W(WHITE)"),
    Case("general_flat", 513, 8, 16, f"C(1.3) * RBF({_LS8}) + W(WHITE) + C(0.2)"),
    # ---- the general path, kernel trees: k_grad_contract<true, 1>
    Case("general_tree", 129, 1, 5, "Pow(C(1.1) * RQ(length_scale=1.2, alpha=0.7) + C(0.5), 2) + W(WHITE)"),
    Case("general_tree", 257, 2, 5, "C(0.6) * RBF([0.8, 1.2]) + C(0.05) * Dot(sigma_0=1.3) + W(WHITE)"),
    # ---- the general path on wide uniform grids (the RBF and Matern-5/2 grids of tests/build_classes.py): dR_p is mostly exact zeros (exp
    # argument below -745.2) and partly subnormal (the band down from -707.7), on 4 resp. 11 diagonals.  n = 278 and 488 are the smallest
    # orders at which a tenth of the entries is in range, a tenth is far and a thousand lie in the band (test_build_classes_cpu.py).
    # Inputs chosen for REF_LIMIT: these matrices are so well conditioned (cond_2(R) = 27 resp. 5 with an amplitude and white noise alone; the
    # Matern grid's points are a length scale apart and no amplitude moves it past 14) that cond S no longer covers the plain einsum
    # reference's ~100 eps S on the dense amplitude and noise parameters (7 resp. 21 eps).  The RBF case carries an additive constant
    # (cond 3e2 on the tight run); the Matern case keeps the one parameter this is about, the length scale
    Case("general_wide", 278, 1, 5, "C(1.3) * RBF(0.2) + W(WHITE) + C(0.5)", grid=0.05),
    Case("general_wide", 488, 1, 5, "Matern(0.3, nu=2.5) + W(WHITE, noise_level_bounds='fixed')", grid=0.3),
]
RUNS = [("tight", WHITE_TIGHT), ("amplified", WHITE_AMPLIFIED)]
CASE_RUNS = [(c, run, w) for c in CASES for run, w in RUNS]
CASE_RUN_IDS = [f"{c.id}-{run}" for c, run, _ in CASE_RUNS]

_TRUTHS = {}


def case_truth(case: Case, run, white):
    """(kernel, X, R, dR, Z_random, Z_selector, cols, Truth) of a case and run: one truth evaluation, shared by the two kinds of right-hand
    sides and by every test of a session (read-only)."""
    key = (case.id, run)
    if key not in _TRUTHS:
        kern, X, R, dK, Z, cols = case.matrices(white)
        Zs = np.ascontiguousarray(R[:, cols])
        T = pieces_truth(R, dK)
        add_rhs(T, "random", Z)
        add_rhs(T, "selector", Zs)
        T.Rinv = T.L = T.dR = None            # (the n x n long-double arrays are not needed again)
        for a in (X, R, dK, Z, Zs):
            a.setflags(write=False)
        _TRUTHS[key] = (kern, X, R, dK, Z, Zs, cols, T)
    return _TRUTHS[key]
