"""Shared cases of the banded likelihood path (test_banded_cpu.py on backend='cpu', test_gpu_banded.py on 'hip'); DESIGN.md section 26.

(a) Exact factors: L of band b with the diagonal 2^e, e in -2 .. 2, and off-diagonals k / 8, k in -3 .. 3; A = L L^T and Z = L Y0 with
    integer Y0 in -3 .. 3 are formed without a rounding (checked in int64), every partial sum of the factorisation, of the substitution
    and of the Gram matrix is a multiple of 2^-6 far below 2^53 of them, so L, Y and G = Y0^T Y0 come back bit for bit in every order.
    sum_log_diag: within 64 * 2^-53 * max(1, |sld|) of ln 2 * sum e in long double (the project's floor).
(b) Componentwise bounds (Higham, Accuracy and Stability, Thm 10.3 and 8.5), evaluated in numpy.longdouble from the returned L and Y:
        |A - L L^T| <= gamma_{b+2} |L||L^T| + (b + 2) 2^-1074
        |Z - L Y|   <= gamma_{b+1} |L||Y|   + (b + 1) 2^-1074
        |G - Y^T Y| <= gamma_{n+1} |Y|^T|Y|
(c) The model value against a band Cholesky of the same band in numpy.longdouble, at 1e-10 relative (the project's bound).
Every check takes the backend and returns what it measured, so the GPU tests can record it."""
import functools

import numpy as np

import gsum_amd as gm

LD = np.longdouble
EPS = 2.0 ** -53
FLOOR = 64 * EPS
TINY = LD(2.0) ** -1074
LN2 = LD("0.693147180559945309417232121458176568075500134360255254120680")
BENCH_LS, BENCH_STEP, BENCH_NUGGET = 0.2, 0.1, 1e-10


def gamma(k):
    return LD(k) * LD(EPS) / (1 - LD(k) * LD(EPS))


# ---- layout -----------------------------------------------------------------------------------------------------------------------------
def to_band(A, b):
    n = A.shape[0]
    AB = np.zeros((b + 1, n), dtype=A.dtype)
    for k in range(min(b, n - 1) + 1):
        AB[k, :n - k] = np.diagonal(A, -k)
    return AB


def to_dense(AB):
    """the lower triangle of the band as an n x n array"""
    b1, n = AB.shape
    A = np.zeros((n, n), dtype=AB.dtype)
    for k in range(min(b1, n)):
        A[np.arange(k, n), np.arange(n - k)] = AB[k, :n - k]
    return A


def widen(AB, extra):
    return np.concatenate([AB, np.zeros((extra, AB.shape[1]))], axis=0)


# ---- (a) exact factors ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(n, b, seed=0):
    """(L band, A band, e) of an exactly representable factor of order n and half-bandwidth b (read-only)."""
    rng = np.random.default_rng([n, b, seed])
    e = rng.integers(-2, 3, size=n)
    L = np.tril(rng.integers(-3, 4, size=(n, n)) / 8.0, -1)
    i, j = np.indices((n, n))
    L[i - j > b] = 0.0
    L[np.arange(n), np.arange(n)] = np.ldexp(1.0, e)
    Li = np.rint(L * 8).astype(np.int64)
    A = L @ L.T
    assert np.array_equal(A * 64.0, (Li @ Li.T).astype(float)) and np.abs(Li @ Li.T).max() < 2 ** 40
    Lb, Ab = to_band(L, b), to_band(A, b)
    assert np.array_equal(np.tril(A), to_dense(Ab))                   # nothing of A lies outside the band
    for a in (Lb, Ab, e):
        a.setflags(write=False)
    return Lb, Ab, e


@functools.lru_cache(maxsize=None)
def exact_rhs(n, b, cols, seed=0):
    """(Z = L Y0, Y0) with integer Y0 (n, cols) in -3 .. 3"""
    Lb = exact_case(n, b, seed)[0]
    Y0 = np.random.default_rng([n, cols, seed + 1]).integers(-3, 4, size=(n, cols)).astype(float)
    L = to_dense(Lb)
    Z = L @ Y0
    assert np.array_equal(Z * 8.0, np.rint(L * 8) @ Y0)
    Z.setflags(write=False)
    Y0.setflags(write=False)
    return Z, Y0


def exact_sizes(b, B):
    return sorted({n for n in (1, 2, b, b + 1, b + 2, 2 * B - 1, 2 * B, 2 * B + 1, 3 * b + 5) if n >= 1})


def exact_widths(B, W):
    return sorted({0, 1, 15, 16, 17, B - 1, B, B + 1, W})


def sld_truth(e):
    return LD(int(np.sum(e))) * LN2


def check_sld(sld, e):
    t = sld_truth(e)
    err = abs(LD(sld) - t)
    assert err <= LD(FLOOR) * max(LD(1), abs(t)), (float(sld), float(t), float(err))
    return float(err)


def check_exact(backend, n, b, cols, n_sets, device=None):
    """(a) for one shape: L, Y, G bit for bit, info 0, sld within the floor; returns the sld error."""
    Lb, Ab, e = exact_case(n, b)
    Z, Y0 = exact_rhs(n, b, cols * n_sets)
    G, sld, info, L = gm.banded_gram(Ab, Z, n_sets, return_factor=True, backend=backend, device=device)
    assert info == 0
    np.testing.assert_array_equal(L, Lb)
    np.testing.assert_array_equal(gm.banded_forward(L, Z, backend=backend, device=device), Y0)
    Ys = Y0.reshape(n, n_sets, cols)
    np.testing.assert_array_equal(G, np.einsum("nsa,nsb->sab", Ys, Ys))
    return check_sld(sld, e)


# ---- long-double band Cholesky (the truth of (c)) -----------------------------------------------------------------------------------------
def ld_band_cholesky(AB):
    """L (b + 1, n) in numpy.longdouble of the band AB, right-looking, column by column; raises where a pivot is not positive."""
    b1, n = AB.shape
    b = b1 - 1
    W = np.array(AB, dtype=LD)
    S, T = np.tril_indices(b) if b else (np.zeros(0, int), np.zeros(0, int))
    for j in range(n):
        p = W[0, j]
        if not p > 0:
            raise np.linalg.LinAlgError(f"pivot {j + 1} is not positive")
        l = np.sqrt(p)
        W[0, j] = l
        kb = min(b, n - 1 - j)
        if kb == 0:
            continue
        col = W[1:kb + 1, j] / l
        W[1:kb + 1, j] = col
        keep = S < kb
        s, t = S[keep], T[keep]
        W[s - t, j + 1 + t] -= col[s] * col[t]
    for k in range(1, b1):
        W[k, max(n - k, 0):] = 0
    return W


def ld_forward(L, Z):
    b1, n = L.shape
    Y = np.zeros(Z.shape, dtype=LD)
    Zl = np.asarray(Z, dtype=LD)
    for i in range(n):
        k = np.arange(1, min(b1 - 1, i) + 1)
        acc = Zl[i]
        if k.size:
            acc = acc - L[k, i - k] @ Y[i - k]
        Y[i] = acc / L[0, i]
    return Y


def ld_gram(AB, Z, n_sets=1):
    """(G (n_sets, c, c), sum_log_diag) of the band in long double, rounded to fp64"""
    L = ld_band_cholesky(AB)
    Y = ld_forward(L, Z).reshape(AB.shape[1], n_sets, -1)
    return np.einsum("nsa,nsb->sab", Y, Y).astype(float), float(np.sum(np.log(L[0])))


# ---- (b) derived bounds -----------------------------------------------------------------------------------------------------------------
def _ratio(resid, bound):
    """max resid / bound; an entry whose bound is zero must have no residual"""
    assert np.all(resid[bound == 0] == 0)
    ok = bound > 0
    return float(np.max(resid[ok] / bound[ok])) if np.any(ok) else 0.0


def bound_ratios(AB, L, Z, Y, G, n_sets=1):
    """The worst ratio residual / bound of each of the three bounds of (b), in long double, for one matrix."""
    b1, n = AB.shape
    b = b1 - 1
    A, Ll, Yl, Zl = (np.asarray(x, dtype=LD) for x in (AB, L, Y, Z))
    La = np.abs(Ll)
    P = np.zeros((b1, n), dtype=LD)                                  # (L L^T)[j + k, j] = sum_d L[j + k, j - d] L[j, j - d]
    Pa = np.zeros((b1, n), dtype=LD)
    for k in range(b1):
        for d in range(b1 - k):
            cols = np.arange(d, n - k)                               # j with j - d >= 0 and j + k < n
            if cols.size:
                P[k, cols] += Ll[d + k, cols - d] * Ll[d, cols - d]
                Pa[k, cols] += La[d + k, cols - d] * La[d, cols - d]
    inside = np.arange(n)[None, :] + np.arange(b1)[:, None] < n
    r1 = _ratio(np.abs(A - P)[inside], (gamma(b + 2) * Pa + (b + 2) * TINY)[inside])
    LY = np.zeros(Zl.shape, dtype=LD)
    LYa = np.zeros(Zl.shape, dtype=LD)
    Ya = np.abs(Yl)
    for d in range(b1):
        rows = np.arange(d, n)
        LY[rows] += Ll[d, rows - d, None] * Yl[rows - d]
        LYa[rows] += La[d, rows - d, None] * Ya[rows - d]
    r2 = _ratio(np.abs(Zl - LY), gamma(b + 1) * LYa + (b + 1) * TINY)
    Ys, Yas = Yl.reshape(n, n_sets, -1), Ya.reshape(n, n_sets, -1)
    r3 = _ratio(np.abs(np.asarray(G, dtype=LD) - np.einsum("nsa,nsb->sab", Ys, Ys)), gamma(n + 1) * np.einsum("nsa,nsb->sab", Yas, Yas))
    return r1, r2, r3


def check_bounds(backend, name, AB, Z, n_sets=1, device=None):
    G, sld, info, L = gm.banded_gram(AB, Z, n_sets, return_factor=True, backend=backend, device=device)
    assert info == 0, info
    Y = gm.banded_forward(L, Z, backend=backend, device=device)
    r = bound_ratios(AB, L, Z, Y, G, n_sets)
    print(f"banded bounds {backend} {name}: factor {r[0]:.3g}, substitution {r[1]:.3g}, gram {r[2]:.3g} of the bound")
    assert max(r) <= 1.0, r
    return r


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def bench_kernel(ls=BENCH_LS):
    from sklearn.gaussian_process.kernels import RBF
    return RBF(ls)


def tree_kernel():
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel as C, Matern, WhiteKernel
    return C(1.5) * Matern(0.05, nu=2.5) + C(0.5) * RBF(0.1) + WhiteKernel(1e-3)


def uniform_points(n):
    return BENCH_STEP * np.arange(n)


@functools.lru_cache(maxsize=None)
def clustered_points(n, seed=0):
    """sorted, not uniform: duplicates, clusters, and gaps wider than the range of every kernel here"""
    rng = np.random.default_rng([n, seed])
    steps = rng.choice([0.0, 0.05, 0.2, 0.5], size=n, p=[0.15, 0.35, 0.3, 0.2])
    steps[rng.choice(n, size=max(n // 60, 1), replace=False)] = 40.0
    X = np.cumsum(steps)
    X.setflags(write=False)
    return X


def rough_curves(AB, cols, seed=0, backend="cpu"):
    """[cols - 1 curves drawn from the band's own process | 1]: L w with the cpu backend's factor"""
    n = AB.shape[1]
    L = gm.banded_gram(AB, np.ones((n, 1)), return_factor=True, backend="cpu")[3]
    Ld = to_dense(L) if n <= 4096 else None
    w = np.random.default_rng(seed).standard_normal((n, cols - 1))
    if Ld is not None:
        y = Ld @ w
    else:
        y = np.zeros((n, cols - 1))
        for d in range(L.shape[0]):
            y[d:] += L[d, :n - d, None] * w[:n - d]
    return np.column_stack([y, np.ones(n)])


def brute_halfwidth(K):
    """the half-bandwidth of a dense matrix: the largest |i - j| of an entry whose bits are not +-0"""
    i, j = np.nonzero((np.asarray(K).view(np.uint64) << np.uint64(1)) != 0)
    return int(np.max(np.abs(i - j))) if i.size else 0


def rows_contiguous(K):
    """in every row the entries that are not +-0 form one run (the premise of the width search)"""
    nz = (np.ascontiguousarray(K).view(np.uint64) << np.uint64(1)) != 0
    return all(np.all(np.diff(np.nonzero(r)[0]) == 1) for r in nz)


def length_scale_at_width(make, X, W, **kw):
    """(ls_in, ls_out): two adjacent-in-bisection length scales of make(ls) on X whose half-bandwidths are W and W + 1"""
    def width(ls):
        try:
            return gm.banded_halfwidth(make(ls), X, **kw)
        except ValueError as exc:
            assert "half-bandwidth exceeds" in str(exc)
            return W + 1
    lo, hi = 1e-3, 1e3                                               # width(lo) <= W < width(hi)
    assert width(lo) <= W < width(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if width(mid) <= W:
            lo = mid
        else:
            hi = mid
    assert width(lo) == W
    return lo, hi


# ---- failures ---------------------------------------------------------------------------------------------------------------------------
def failing_band(Ab, Lb, p, nan=None):
    """A with A[p, p] lowered by 2 L_pp^2 (pivot p exactly -L_pp^2); nan = (k, j): a NaN at AB[k, j] instead"""
    A = np.array(Ab)
    if nan is None:
        A[0, p] -= 2.0 * Lb[0, p] ** 2
    else:
        A[nan] = np.nan
    return A


def check_failures(backend, B, device=None):
    """info of matrices that do not factor, in one call around two unedited ones, which come out bit for bit as alone"""
    n, b = 3 * B + 5, B + 3
    Lb, Ab, e = exact_case(n, b)
    Z, Y0 = exact_rhs(n, b, 3)
    ps = sorted({0, 1, B - 1, B, B + 1, n - 2, n - 1})
    # AB[k, j] = A[j + k, j] enters column j of L below the diagonal and pivot j + k first: info j + k + 1
    nans = [((0, B + 2), B + 3), ((2, 5), 8), ((b, 1), b + 2), ((1, 2 * B - 1), 2 * B + 1)]
    mats = [Ab] + [failing_band(Ab, Lb, p) for p in ps] + [failing_band(Ab, Lb, 0, nan=pos) for pos, _ in nans] + [Ab]
    want = [0] + [p + 1 for p in ps] + [w for _, w in nans] + [0]
    G, sld, info = gm.banded_gram(np.stack(mats), Z, backend=backend, device=device)
    assert list(info) == want, (list(info), want)
    G0, s0, i0 = gm.banded_gram(Ab, Z, backend=backend, device=device)
    assert i0 == 0
    for i, w in enumerate(want):
        if w == 0:
            assert np.array_equal(G[i], G0) and sld[i] == s0
        else:
            assert np.isnan(G[i]).all() and np.isnan(sld[i])
    return want


# ---- (c) the model layer ----------------------------------------------------------------------------------------------------------------
def model_process(backend, kernel=None, **kw):
    return gm.ConjugateGaussianProcess(kernel=bench_kernel() if kernel is None else kernel, center=0.1, disp=1.5, df=2, scale=0.7,
                                       nugget=BENCH_NUGGET, optimizer=None, backend=backend, **kw)


def truncation_process(backend, X, y, orders=3, **kw):
    """a TruncationGP on the benchmark's kernel with the first ``orders`` curves of y as coefficients"""
    tg = gm.TruncationGP(kernel=bench_kernel(), ratio=0.5, ref=1.0, optimizer=None, nugget=BENCH_NUGGET, backend=backend, **kw)
    tg.X_train_, tg.y_train_, tg.orders_ = X, gm.partials(y[:, :orders], ratio=0.5, ref=1.0, orders=np.arange(orders)), np.arange(orders)
    return tg


MODEL_THETAS = (np.log([0.2]), np.log([0.12]), np.log([0.19]))           # the second has a smaller half-bandwidth than the others
MODEL_RATIOS = (0.3, 0.4, 0.5, 0.6)


def check_model(backend, n):
    """(c) at order n: single, batch and grid entries bit for bit; the value against the long-double truth (1e-10) and against the
    dense route (2e-10).  Returns (worst distance from the truth, worst distance from the dense route)."""
    X, y = model_inputs(n)
    gp = model_process(backend)
    thetas = list(MODEL_THETAS)
    vals = gp.log_marginal_likelihood_batch(thetas, X=X, y=y, structure="banded")
    assert vals.shape == (3,) and np.all(np.isfinite(vals))
    widths = gm.banded_halfwidth([gp.kernel.clone_with_theta(t) for t in thetas], X, backend=backend)
    assert widths[1] < widths[0]
    d_truth = d_dense = 0.0
    for t, v in zip(thetas, vals):
        assert gp.log_marginal_likelihood(t, X=X, y=y, structure="banded") == v
        assert gp.log_marginal_likelihood_batch([t], X=X, y=y, structure="banded")[0] == v
        truth = truth_value(gp, gp.kernel.clone_with_theta(t), X, y)
        dense = gp.log_marginal_likelihood(t, X=X, y=y)
        print(f"banded model {backend} n={n} theta={t[0]:.3f}: truth {rel(v, truth):.3g}, dense {rel(v, dense):.3g} (dense to truth {rel(dense, truth):.3g})")
        d_truth, d_dense = max(d_truth, rel(v, truth)), max(d_dense, rel(v, dense))
    assert d_truth <= 1e-10 and d_dense <= 2e-10, (d_truth, d_dense)
    tg = truncation_process(backend, X, y)
    ratios = list(MODEL_RATIOS)
    grid = tg.log_marginal_likelihood_grid(thetas, ratios, structure="banded")
    assert grid.shape == (4, 3) and np.all(np.isfinite(grid))
    assert np.array_equal(grid, tg.log_marginal_likelihood_grid(thetas, ratios, structure="banded", mode="reuse"))
    for i, j in ((0, 0), (3, 1), (2, 2)):
        assert tg.log_marginal_likelihood_grid([thetas[j]], [ratios[i]], structure="banded")[0, 0] == grid[i, j]
    dg = float(np.max(np.abs(grid - tg.log_marginal_likelihood_grid(thetas, ratios)) / np.maximum(1.0, np.abs(grid))))
    print(f"banded grid {backend} n={n}: dense {dg:.3g}")
    assert dg <= 2e-10
    half = np.concatenate([tg.log_marginal_likelihood_grid(thetas, ratios, structure="banded", shard=(r, 2))[:, None] for r in (0, 1)], axis=1)
    assert np.array_equal(np.where(np.isnan(half[:, 0]), half[:, 1], half[:, 0]), grid)
    return d_truth, max(d_dense, dg)


@functools.lru_cache(maxsize=None)
def model_inputs(n, curves=5):
    """(X (n, 1), y (n, curves)) on the benchmark's grid: curves drawn from the kernel itself"""
    X = uniform_points(n)[:, None]
    AB = gm.banded_matrix(bench_kernel(), X, nugget=BENCH_NUGGET, backend="cpu")
    y = rough_curves(AB, curves + 1)[:, :curves]
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def truth_value(gp, kernel, X, y):
    """the log marginal likelihood from the long-double band Cholesky of the cpu backend's band, through the process's host algebra"""
    AB = gm.banded_matrix(kernel, X, nugget=gp.nugget, backend="cpu")
    Z = gp._rhs(np.asarray(X), y)
    G, sld = ld_gram(AB, Z)
    return float(gp._lml_gram(G[0], sld, X.shape[0])[0])


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))
