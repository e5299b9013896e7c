"""Long-double truth, error scales and the case matrices for the predictive pieces of gsum_predict_terms[_series] and for the series
scaling k_scale_series behind its three entry points (no tests here; tests/test_predict_truth_cpu.py and tests/test_gpu_predict_truth.py).
Constants and the protocol are those of tests/grad_truth.py:  e_dev <= BOUND max(e_ref, eps),  admissible if e_ref <= REF_LIMIT eps.

Predictive pieces.  With the float64 arrays  R = kernel(X) + nugget I  (n x n)  and  Kst = kernel(Xs, X)  (m x n)  taken from the context
under test as EXACT inputs (the device's exp is not numpy's), and right-hand sides Z (n x 16):
    L = cholesky_ld(R),  Rinv = L^-T L^-1,  B = [Kst^T | Z],  Gt = B^T Rinv B      (numpy.longdouble)
    colsumsq = diag of the Kst block,   cov = the Kst block,   VtW = the Kst x Z block
    S = |B|^T |Rinv| |B|  (grad_truth's S_G),   e(x) = max |x - truth| / (cond_2(R) S).

Series scaling.  One entry of  A_ij *= factor ref_r[i] ref_c[j] S(x),  x = fl(ratio_r[i] ratio_c[j])  (the kernel forms exactly this product:
x is an exact input), in long double:
    S(x) = (x^start - x^(end+1)) / (1 - x) - sum_{e excluded, start <= e <= end} x^e           (x^(end+1) = 0 for an infinite sum)
    truth = (ref_r[i] ref_c[j]) S(x) (factor A_ij),    scale = |ref_r ref_c| s(x) |factor A_ij|,
    s(x) = (|x|^start + |x|^(end+1)) / |1 - x| + sum |x|^e        -- it carries the cancellation next to x = 1 that numpy's expression has too.
Entries with x == 1 exactly are 0 / 0 in the float64 reference: the device must return the same class there (nan, +inf, -inf); they are
planted on purpose, counted, and are the only entries left out of the error maximum."""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

import grad_truth as gt

LD = gt.LD
EPS = gt.EPS
NUGGET = gt.NUGGET
RUNS = gt.RUNS                                   # ("tight", WHITE_TIGHT), ("amplified", WHITE_AMPLIFIED)
MAX_RHS = 16                                     # GSUM_MAX_RHS
MAX_EXCLUDED = 16                                # GSUM_MAX_EXCLUDED
PIECES = ("colsumsq", "cov", "VtW")

# ---- part 1: the predictive pieces -------------------------------------------------------------------------------------------------
# (n, m): n = 1, 127, 128 -> one block column (no trailing update); 129, 256 -> one pair; 257 -> a pair and a single block; 385 -> two pairs;
# 513 -> five block columns (odd, K = 256 trailing update).  Every m of {1, 2, 7, 9, 15, 17, 129} occurs with T = 1 and with T >= 3:
# 1, 2, 7, 9 around k_rowsumsq_vw's two rows per wave / eight per workgroup and k_rowsumsq's four per workgroup, 15, 17 around k_panel256's
# 16 rows per wave, 129 past the 128-row GEMM tile and the lower-tile V^T V.
SHAPES = [(1, 1), (1, 17), (127, 2), (127, 7), (127, 129), (128, 9), (128, 15),
          (129, 2), (129, 9), (256, 7), (256, 17),
          (257, 1), (257, 15), (257, 17), (385, 2), (385, 129), (513, 7), (513, 9)]
SHAPE_RUNS = [(n, m, run, white) for n, m in SHAPES for run, white in RUNS]
SHAPE_RUN_IDS = [f"n{n}-m{m}-{run}" for n, m, run, _ in SHAPE_RUNS]


def block_columns(n):
    return (n + 127) // 128


def check_shape_coverage():
    for m in (1, 2, 7, 9, 15, 17, 129):
        ts = [block_columns(n) for n, mm in SHAPES if mm == m]
        assert 1 in ts and max(ts) >= 3, (m, ts)
    assert sorted({n for n, _ in SHAPES}) == [1, 127, 128, 129, 256, 257, 385, 513]


def kernel(white):
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    return Matern([0.7, 1.3], nu=2.5) + WhiteKernel(white)


def points(n, m):
    """Conditioning points (a function of n alone), m new points with distinct rows, and Z = [randn(n, 15) | 1]: asymmetric, so that a
    swapped row or column map cannot cancel."""
    side = np.array([0.35, 0.65]) * np.sqrt(n)
    rng = np.random.RandomState(1000 + n)
    X = rng.rand(n, 2) * side
    Z = np.concatenate([rng.randn(n, MAX_RHS - 1), np.ones((n, 1))], axis=1)
    Xs = np.random.RandomState(zlib.crc32(f"{n}x{m}".encode()) & 0x7FFFFFFF).rand(m, 2) * side
    return X, Xs, Z


@dataclass
class PredictTruth:
    cond: float
    m: int
    Gt: np.ndarray          # (m + 16, m + 16) longdouble
    S: np.ndarray

    def piece(self, name, cols=None):
        m = self.m
        if name == "colsumsq":
            return np.diag(self.Gt)[:m], np.diag(self.S)[:m]
        if name == "cov":
            return self.Gt[:m, :m], self.S[:m, :m]
        c = slice(m, m + MAX_RHS) if cols is None else m + np.asarray(cols)
        return self.Gt[:m, c], self.S[:m, c]

    def errors(self, colsumsq, VtW, cov, cols=None):
        """Normalised error of each piece handed in (None: not asked for); ``cols``: which columns of Z the VtW handed in belongs to."""
        out = {}
        for name, x in (("colsumsq", colsumsq), ("cov", cov), ("VtW", VtW)):
            if x is not None:
                t, s = self.piece(name, cols)
                assert np.shape(x) == t.shape, (name, np.shape(x), t.shape)
                out[name] = gt.normalised_error(x, t, self.cond, s)
        return out


_RINV, _TRUTH = {}, {}


def predict_truth(tag, R, Kst, Z):
    """Truth for exact inputs R, Kst, Z.  ``tag`` names where R came from (backend, n, run, ...): R^-1 in long double is evaluated once per
    tag and shared by every m; a tag must always come with the same R."""
    gt._require_extended()
    R, Kst, Z = (np.asarray(a, dtype=np.float64) for a in (R, Kst, Z))
    n, m = len(R), len(Kst)
    assert R.shape == (n, n) and Kst.shape == (m, n) and Z.shape == (n, MAX_RHS)
    if tag not in _RINV:
        Li = gt.inverse_lower_ld(gt.cholesky_ld(R))
        _RINV[tag] = (R.copy(), Li.T @ Li, float(np.linalg.cond(R)))
    R0, Rinv, cond = _RINV[tag]
    assert np.array_equal(R0, R), f"tag {tag!r} was used with another matrix"
    key = (tag, m, zlib.crc32(Kst.tobytes()), zlib.crc32(Z.tobytes()))
    if key not in _TRUTH:
        B = np.concatenate([Kst.T, Z], axis=1).astype(LD)
        aB = np.abs(B)
        _TRUTH[key] = PredictTruth(cond=cond, m=m, Gt=B.T @ (Rinv @ B), S=aB.T @ (np.abs(Rinv) @ aB))
    return _TRUTH[key]


def reference_pieces(R, Kst, Z):
    """The plain float64 evaluation on the same inputs: numpy.linalg.cholesky, solve_triangular, einsum -> colsumsq, VtW, cov."""
    from scipy.linalg import solve_triangular
    L = np.linalg.cholesky(R)
    V = solve_triangular(L, Kst.T, lower=True)
    W = solve_triangular(L, Z, lower=True)
    return np.einsum("ij,ij->j", V, V), V.T @ W, V.T @ V


VARIANTS = [("none", None), ("k1", [0]), ("k16", list(range(MAX_RHS)))]      # rhs=None (k_rowsumsq); one column; GSUM_MAX_RHS with the constant


def evaluate_pieces(ctx, tag, n, m, white, series=None, diag_add=NUGGET, variants=VARIANTS, covs=(False, True)):
    """Every call variant of one shape on ``ctx`` (HipContext or CpuContext) against the truth for the context's OWN kernel matrices.
    Returns (truth, e_ref, calls): e_ref by piece, calls = [(label, e_dev by piece, (colsumsq, VtW, cov))].  ``series`` =
    (SeriesScale, ref_x, ratio_x, ref_s, ratio_s) scales R and Kst like TruncationProcess.cov."""
    import gsum_amd
    X, Xs, Z = points(n, m)
    desc = gsum_amd.describe_kernel(kernel(white), 2)
    if series is None:
        R = ctx.kernel_matrix(desc, X, diag_add=diag_add)
        Kst = ctx.kernel_matrix(desc, Xs, X)
        L, info = ctx.factorize(desc, X, diag_add=diag_add)
    else:
        sc, ref_x, ratio_x, ref_s, ratio_s = series
        R = ctx.kernel_matrix(desc, X, diag_add=diag_add, series=(sc, ref_x, ratio_x))
        Kst = ctx.kernel_matrix(desc, Xs, X, series=(sc, ref_s, ratio_s, ref_x, ratio_x))
        L, info = ctx.factorize(desc, X, diag_add=diag_add, series=(sc, ref_x, ratio_x))
    assert info == 0 and Kst.shape == (m, n)
    try:
        T = predict_truth(tag, R, Kst, Z)
        e_ref = T.errors(*reference_pieces(R, Kst, Z))
        calls = []
        for name, cols in variants:
            for want_cov in covs:
                rhs = None if cols is None else np.ascontiguousarray(Z[:, cols])
                got = ctx.predict_terms(L, desc, X, Xs, rhs=rhs, want_cov=want_cov, series=series)
                assert (got[1] is None) == (cols is None) and (got[2] is None) == (not want_cov)
                calls.append((f"{name}{'-cov' if want_cov else ''}", T.errors(*got, cols=cols), got))
    finally:
        L.free()
    return T, e_ref, calls


def over_bound(label, e_ref, calls):
    """The calls and pieces that miss  e_dev <= BOUND max(e_ref, eps)  (empty: fine), and the worst e_dev by piece."""
    over, worst = [], {}
    for name, e_dev, _ in calls:
        for piece, e in e_dev.items():
            worst[piece] = max(worst.get(piece, 0.0), e)
            if not e <= gt.BOUND * max(e_ref[piece], EPS):
                over.append(f"{label}/{name}/{piece}: e_dev {e / EPS:.3g} eps, e_ref {e_ref[piece] / EPS:.3g} eps")
    return over, worst


def exact_properties(calls):
    """cov is bit-symmetric and the same bits whatever right-hand sides came with it; VtW of column 0 is the same bits between k = 1 and
    k = 16; colsumsq and VtW do not depend on want_cov.  (diag(cov) == colsumsq need not hold: other summation orders; nor need the
    colsumsq of k_rowsumsq and of k_rowsumsq_vw agree in the last bit.)"""
    by = {name: got for name, _, got in calls}
    for name, (css, vtw, cov) in by.items():
        if cov is not None:
            assert np.array_equal(cov, cov.T), f"{name}: cov is not bit-symmetric"
            assert np.array_equal(cov, by["none-cov"][2]), f"{name}: cov depends on the right-hand sides"
    assert np.array_equal(by["k1"][1][:, 0], by["k16"][1][:, 0]), "VtW column 0 depends on the other columns passed"
    for k in ("none", "k1", "k16"):
        assert np.array_equal(by[k][0], by[k + "-cov"][0]), f"{k}: colsumsq depends on want_cov"
        if k != "none":
            assert np.array_equal(by[k][1], by[k + "-cov"][1]), f"{k}: VtW depends on want_cov"


# ---- part 2: series scaling --------------------------------------------------------------------------------------------------------
INF = np.inf
# (start, end, excluded, factor)
SERIES = {
    "0-inf": (0, INF, [], 1.0),
    "3-inf-x2,4": (3, INF, [2, 4], 1.0),                                         # 2 < start: ignored
    "1-4-x2": (1, 4, [2], 1.0),
    "0-60-x0,7,60": (0, 60, [0, 7, 60], 1.0),
    "5-5": (5, 5, [], 1.0),
    "2-40-x16": (2, 40, [2, 3, 5, 8, 13, 21, 34, 39, 40, 41, 55, 60, 0, 1, 100, 7], 1.0),     # GSUM_MAX_EXCLUDED orders, six outside [2, 40]
    "0-8-x3-f": (0, 8, [3], -0.37),
}
REGIMES = ("mid", "signed", "near_one", "above_one")


def series_configs(regime):
    """above one: finite sums only (an infinite geometric sum diverges there)."""
    return [k for k, v in SERIES.items() if regime != "above_one" or np.isfinite(v[1])]


def series_scale(name):
    from gsum_amd._lib import SeriesScale
    start, end, exc, factor = SERIES[name]
    assert len(exc) <= MAX_EXCLUDED
    return SeriesScale.make(start, end, exc or None, factor)


def _regime_values(rng, regime, size):
    if regime == "mid":
        return 0.3 + 0.4 * rng.rand(size)
    if regime == "signed":
        return -0.9 + 1.8 * rng.rand(size)
    if regime == "near_one":
        return 1.0 - 2.0 ** -rng.randint(8, 27, size=size).astype(float)
    assert regime == "above_one"
    return 1.0 + rng.rand(size)


# planted ratios, by priority as far as a vector's length reaches.  "unit": the x == 1 entry -- for a finite sum the pair 2.0 (rows) x 0.5
# (columns; both in a symmetric call), for an infinite sum, where 2.0 would put a diverging x > 1 beside it, the ratio 1.0 on both sides.
# 0.0: x = 0 (0^0 = 1 for start = 0, S = 0 for start > 0).  1e-6: with end = 60 its powers run through the subnormal range to zero.
# 2.9e-3: squared, x = 8.41e-6, whose power 61 (1.3e-310) IS subnormal while its power 60 is not.
def vectors(regime, config, n_rows, n_cols=None, seed=0):
    """(ref_r, ratio_r, ref_c, ratio_c, planted): ``planted`` = the number of entries with x == 1 exactly.  n_cols None: a symmetric call
    (one vector for both sides)."""
    finite = np.isfinite(SERIES[config][1])
    rng = np.random.RandomState(zlib.crc32(f"{regime}/{config}/{n_rows}/{n_cols}/{seed}".encode()) & 0x7FFFFFFF)

    def one(size, side):
        ref = rng.choice([-1.0, 1.0], size=size) * 10.0 ** (-1.0 + 2.0 * rng.rand(size))          # mixed sign, 0.1 ... 10
        ratio = _regime_values(rng, regime, size)
        unit = ((2.0, 0.5) if side == "both" else (2.0,) if side == "rows" else (0.5,)) if finite else (1.0,)
        # eight values or more: every plant; fewer: the unit entry alone where it leaves a value of the regime; one value: the regime's
        plants = list(unit) + [0.0, 1e-6, 2.9e-3] if size >= 8 else list(unit) if len(unit) < size else []
        where = [size - 1, 0, size // 2, size // 3, (2 * size) // 3]
        for value, pos in zip(plants, where):
            ratio[pos] = value
        return ref, ratio, plants

    if n_cols is None:
        ref, ratio, placed = one(n_rows, "both")
        planted = (2 if finite else 1) if (all(v in placed for v in (2.0, 0.5)) if finite else 1.0 in placed) else 0
        return ref, ratio, ref, ratio, planted
    ref_r, ratio_r, pr = one(n_rows, "rows")
    ref_c, ratio_c, pc = one(n_cols, "cols")
    planted = int(((2.0 in pr and 0.5 in pc) if finite else (1.0 in pr and 1.0 in pc)))
    return ref_r, ratio_r, ref_c, ratio_c, planted


def series_truth(config, A, ref_r, ratio_r, ref_c, ratio_c):
    """(truth, scale, unit): long-double truth and error scale per entry of the scaled A, and the mask of the entries with x == 1."""
    gt._require_extended()
    start, end, exc, factor = SERIES[config]
    x64 = np.asarray(ratio_r, dtype=np.float64)[:, None] * np.asarray(ratio_c, dtype=np.float64)[None, :]       # fl(ratio_r ratio_c)
    unit = x64 == 1.0
    x = np.where(unit, 0.5, x64).astype(LD)
    ax = np.abs(x)
    hi, ahi = (LD(0) * x, LD(0) * x) if np.isinf(end) else (x ** int(end + 1), ax ** int(end + 1))
    S = (x ** int(start) - hi) / (1 - x)
    s = (ax ** int(start) + ahi) / np.abs(1 - x)
    for e in exc:
        if start <= e <= end:
            S = S - x ** int(e)
            s = s + ax ** int(e)
    refm = np.asarray(ref_r, dtype=LD)[:, None] * np.asarray(ref_c, dtype=LD)[None, :]
    fa = LD(factor) * np.asarray(A, dtype=LD)
    return refm * S * fa, np.abs(refm) * s * np.abs(fa), unit


def series_reference(config, A, ref_r, ratio_r, ref_c, ratio_c):
    """The float64 reference on the same inputs: gsum_amd.geometric_sum through the cpu backend's _series_factor."""
    from gsum_amd._cpu import _series_factor
    with np.errstate(all="ignore"):
        return _series_factor(series_scale(config), np.asarray(ref_r, float), np.asarray(ratio_r, float), np.asarray(ref_c, float),
                              np.asarray(ratio_c, float)) * np.asarray(A, dtype=float)


def nonfinite_class(a):
    a = np.asarray(a, dtype=float)
    return np.where(np.isnan(a), 3, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 0)))


def series_errors(config, A, vec, got):
    """(e_dev, e_ref) of a scaled matrix ``got`` for exact input A and vec = vectors(...).  Asserts the non-finite contract: the reference
    is non-finite exactly on the planted x == 1 entries, the result under test is non-finite there, of the same class, and finite elsewhere."""
    ref_r, ratio_r, ref_c, ratio_c, planted = vec
    truth, scale, unit = series_truth(config, A, ref_r, ratio_r, ref_c, ratio_c)
    ref = series_reference(config, A, ref_r, ratio_r, ref_c, ratio_c)
    assert got.shape == ref.shape == truth.shape
    assert int(unit.sum()) == planted, (config, int(unit.sum()), planted)
    assert np.array_equal(~np.isfinite(ref), unit), f"{config}: the reference is non-finite on {int((~np.isfinite(ref)).sum())} entries, {planted} planted"
    assert np.array_equal(nonfinite_class(got), nonfinite_class(ref)), \
        f"{config}: non-finite entries differ: got {got[unit | ~np.isfinite(got)][:4]}, reference {ref[unit | ~np.isfinite(got)][:4]}"
    keep = ~unit
    if not keep.any():
        return 0.0, 0.0
    return (gt.normalised_error(got[keep], truth[keep], 1.0, scale[keep]), gt.normalised_error(ref[keep], truth[keep], 1.0, scale[keep]))


def symmetric_matrix(n, seed=0):
    """A random symmetric float64 matrix of mixed sign (an exact input: no kernel build)."""
    M = np.random.RandomState(7000 + 13 * n + seed).randn(n, n)
    return np.tril(M) + np.tril(M, -1).T


UPLOAD_ORDERS = [1, 255, 256, 257]                      # the grid's 256-column edge; 255 and 257 have identity padding
ONE_ARG_ORDERS = [129, 256]                             # host build: ldo = cols + 1 and ldo = cols
CROSS_SHAPES = [(257, 1), (3, 257), (129, 255)]
ONE_ARG_DIAG_ADD = 0.25
PREDICT_SERIES = [(129, 9), (257, 17)]
PREDICT_SERIES_CONFIGS = ["0-inf", "1-4-x2"]


def series_points(n, m=None):
    side = np.array([0.35, 0.65]) * np.sqrt(max(n, m or 0))
    X = np.random.RandomState(3000 + n).rand(n, 2) * side
    Y = None if m is None else np.random.RandomState(4000 + m).rand(m, 2) * side
    return X, Y


def predict_series_vectors(config, n, m):
    """mid regime without planted entries (R must stay positive definite and every entry finite): ref, ratio on the n conditioning points and
    the m new ones."""
    rng = np.random.RandomState(zlib.crc32(f"predict/{config}/{n}/{m}".encode()) & 0x7FFFFFFF)
    mk = lambda size: (rng.choice([-1.0, 1.0], size=size) * 10.0 ** (-1.0 + 2.0 * rng.rand(size)), 0.3 + 0.4 * rng.rand(size))  # noqa: E731
    (ref_x, ratio_x), (ref_s, ratio_s) = mk(n), mk(m)
    return ref_x, ratio_x, ref_s, ratio_s


SERIES_ENTRIES = ([("upload", (n, None)) for n in UPLOAD_ORDERS] + [("one_arg", (n, None)) for n in ONE_ARG_ORDERS]
                  + [("cross", s) for s in CROSS_SHAPES])
SERIES_ENTRY_IDS = [f"{e}-n{n}" + (f"-m{m}" if m else "") for e, (n, m) in SERIES_ENTRIES]


def series_call(ctx, entry, shape, regime, config):
    """One scaled matrix through entry point ``entry`` of ``ctx``: (A, vec, got) -- the exact unscaled input, vectors(...), the result."""
    with np.errstate(all="ignore"):                  # (the cpu backend's own 0 / 0 at the planted entries)
        return _series_call(ctx, entry, shape, regime, config)


def _series_call(ctx, entry, shape, regime, config):
    import gsum_amd
    n, m = shape
    sc = series_scale(config)
    vec = vectors(regime, config, n, m)
    ref_r, ratio_r, ref_c, ratio_c, _ = vec
    if entry == "upload":
        A = symmetric_matrix(n)
        M = ctx.upload(A)
        try:
            M.scale_series(sc, ref_r, ratio_r)
            return A, vec, M.to_host()
        finally:
            M.free()
    desc = gsum_amd.describe_kernel(kernel(gt.WHITE_TIGHT), 2)
    X, Y = series_points(n, m)
    if entry == "one_arg":
        A = ctx.kernel_matrix(desc, X, diag_add=ONE_ARG_DIAG_ADD)
        got = ctx.kernel_matrix(desc, X, diag_add=ONE_ARG_DIAG_ADD, series=(sc, ref_r, ratio_r))
        M = ctx.kernel_matrix_dev(desc, X, diag_add=ONE_ARG_DIAG_ADD)
        try:
            M.scale_series(sc, ref_r, ratio_r)
            two_steps = M.to_host()
        finally:
            M.free()
        assert np.array_equal(got, two_steps, equal_nan=True), "kernel_matrix(series=) differs from kernel_matrix_dev + scale_series"
        return A, vec, got
    assert entry == "cross"
    A = ctx.kernel_matrix(desc, X, Y)
    return A, vec, ctx.kernel_matrix(desc, X, Y, series=(sc, ref_r, ratio_r, ref_c, ratio_c))


# ---- part 4: the border-row memo ---------------------------------------------------------------------------------------------------
def memo_sequence(ctx, n, m=17):
    """The calls that set, reuse and invalidate a factor's remembered forward solve, each compared bit for bit with the same call on a
    freshly factorised matrix: predict_terms(Z) twice, predict_terms(Z[:, :3]), cho_solve(Z), predict_terms(Z), cho_solve(Z) once more,
    predict_terms(None), forward_gram(Z) + predict_var(want_vtw).  cho_solve gets the SAME right-hand sides as the predict_terms after it:
    its back-substitution overwrites the border rows, and only equal bytes could make a memo that was not dropped pass for valid."""
    import gsum_amd
    X, Xs, Z = points(n, m)
    Z = np.ascontiguousarray(Z[:, :5])
    desc = gsum_amd.describe_kernel(kernel(gt.WHITE_AMPLIFIED), 2)

    def fresh(call):
        L, info = ctx.factorize(desc, X, diag_add=NUGGET)
        assert info == 0
        try:
            return call(L)
        finally:
            L.free()

    def gram_then_var(L):
        G, sld = ctx.forward_gram(L, Z)
        return (G, np.float64(sld)) + tuple(ctx.predict_var(L, desc, X, Xs, want_vtw=True))

    steps = [("predict_terms(Z)", lambda L: ctx.predict_terms(L, desc, X, Xs, rhs=Z, want_cov=True)),
             ("predict_terms(Z) again", lambda L: ctx.predict_terms(L, desc, X, Xs, rhs=Z, want_cov=True)),
             ("predict_terms(Z[:, :3])", lambda L: ctx.predict_terms(L, desc, X, Xs, rhs=np.ascontiguousarray(Z[:, :3]))),
             ("cho_solve(Z)", lambda L: (ctx.cho_solve(L, Z),)),
             ("predict_terms(Z) after cho_solve", lambda L: ctx.predict_terms(L, desc, X, Xs, rhs=Z)),
             ("cho_solve(Z) on the remembered solve", lambda L: (ctx.cho_solve(L, Z),)),
             ("predict_terms(None)", lambda L: ctx.predict_terms(L, desc, X, Xs, rhs=None, want_cov=True)),
             ("forward_gram(Z), predict_var", gram_then_var)]
    L, info = ctx.factorize(desc, X, diag_add=NUGGET)
    assert info == 0
    try:
        for name, call in steps:
            got, want = call(L), fresh(call)
            assert len(got) == len(want)
            for i, (a, b) in enumerate(zip(got, want)):
                assert (a is None) == (b is None), (name, i)
                if a is not None:
                    assert np.all(np.isfinite(a)) and np.array_equal(np.asarray(a), np.asarray(b)), f"n = {n}: {name}: output {i} differs"
    finally:
        L.free()
