"""Entry-by-entry long-double truth for the kernel matrix and its derivative matrices dR_p = d kernel(X) / d log theta_p, the error scale
of one entry, the exactly representable designs and the case matrix (no tests here).

What is pinned.  ``gs_kernel_grad``, ``gs_leaf_dlog_ls``, ``gs_leaf_eval`` and ``gs_tree_eval`` (csrc/kernels/build.hip.h, grad.hip.h)
evaluate dR_p on the fly.  tests/grad_truth.py takes scikit-learn's float64 ``K_gradient`` as exact input and sees the device's entries only
through trace_p and H_p, under a bound scaled by cond_2(R) and a sum over a matrix; here every entry the production kernels computed
(``HipContext.grad_entries``: gsum_debug_grad_entries of the lab build) is compared with the mathematical definition.

Designs.  X lies on the lattice of multiples of 2^-6 with |x| < 64, every length scale (each dimension's included) is a power of two.  A
difference of two coordinates then has at most 13 significant bits, its scaled square at most 26, a sum of eight of them at most 29: the
squared scaled distance s is EXACT in float64 in both device forms ((xi - xj) * inv_ls and xi / ls - xj / ls) and in scikit-learn, and what
separates the device, scikit-learn and the truth is function evaluation (sqrt, exp, pow, log, sin, cos and the arithmetic behind them) and
nothing else.  ``assert_exact_design`` states that (float64 s == long-double s for every pair).  On random points the rounding of x / l
alone moves an entry by hundreds of ulps, which is why random inputs cannot carry a tight bound.

Truth.  ``numpy.longdouble`` (x87: 64-bit mantissa, ``_require_extended``), value and every d / d log parameter from the definition:
    RBF, Matern(inf)   v = exp(-s / 2)                                  d/dlog l_m = D_m v                      (D_m = ((xi_m - xj_m) / l_m)^2, s = sum D_m;
    Matern 1/2         v = exp(-r),  r = sqrt(s)                        D_m v / r   (0 where r = 0)              an isotropic l takes D = s)
    Matern 3/2         v = (1 + t) exp(-t),  t = sqrt(3 s)              3 D_m exp(-t)
    Matern 5/2         v = (1 + t + t^2 / 3) exp(-t),  t = sqrt(5 s)    5/3 D_m (1 + t) exp(-t)
    RationalQuadratic  v = exp(-alpha log1p(u)),  u = q / (2 alpha l^2), q = |xi - xj|^2
                       d/dlog l = q v / (l^2 (1 + u))                   d/dlog alpha = alpha v (u / (1 + u) - log1p(u))
    ExpSineSquared     v = exp(-2 (sin(a) / l)^2),  a = pi |xi - xj| / p   (pi in long double)
                       d/dlog l = 4 sin(a)^2 v / l^2                    d/dlog p = 4 a cos(a) sin(a) v / l^2
    DotProduct         v = xi . xj + sigma_0^2                          d/dlog sigma_0 = 2 sigma_0^2
    ConstantKernel c, WhiteKernel w (on the diagonal of the one-argument form): value and derivative are c resp. w
the one-argument form's diagonal of a stationary leaf is exactly 1 with derivative 0 (np.fill_diagonal), and leaves are composed by the
exact sum, product and power rules (Exponentiation: K^e, dK e K^(e-1)).

Error scale S of an entry: a first-order forward-error model of scikit-learn's float64 formula (kernels.py) -- |truth| plus, for every
rounded intermediate x whose rounding is amplified, |x dg/dx|, the amount by which ONE relative rounding of x moves the result g:
    the exp argument t (s / 2, r, sqrt(3 s), sqrt(5 s), 2 (sin a / l)^2):  g = c exp(-t)  ->  |t| |g|
    ExpSineSquared's a = pi d / p (float64 pi, a product and a quotient):  |a| |dg/da|,  with
        dv/da = -4 sin cos v / l^2,   d(dlog l)/da = 4 / l^2 (2 sin cos v + sin^2 dv/da),
        d(dlog p)/da = 4 / l^2 ((cos sin + a (cos^2 - sin^2)) v + a cos sin dv/da)
        At a zero of sin (|xi - xj| a multiple of the period: ExpSineSquared(0.5, 0.75) on the lattice) dlog l = 4 sin^2 v / l^2 and its
        first-order terms vanish together, while float64 pi leaves sin(a) = 1.2e-16 a / pi there: the SECOND-order move of one rounding
        delta = eps of a, (a delta)^2 / 2 times d2(dlog l)/da2 ~ 8 cos^2 v / l^2, is what remains -- in units of eps:
        eps a^2 / 2 * 8 cos^2 v / l^2.  (Without it scikit-learn's own entries at those pairs are 214 eps of a scale of 1e-33.)
    RationalQuadratic's base = fl(1 + u), whose rounding is an ABSOLUTE ulp(base) / 2 (relative eps / (2 base) in the first binade, which
        is where alpha |v| / base comes from):  |dg/dbase| ulp(base) / eps  with q held fixed as scikit-learn's formula holds it,
        dv/dbase = -alpha v / base,  d(dlog l)/dbase = -(alpha + 1) (dlog l) / base,
        d(dlog alpha)/dbase:  alpha |v| |T| / base + |v| (alpha / base + T2 / base),  T = -T1 + T2,  T1 = alpha log(base), T2 = q / (2 l^2 base);
        and the two terms of that difference, each rounded once:  |v| (T1 + T2)
    where a float64 result underflows its rounding is absolute, half the smallest subnormal = eps DBL_MIN / 2:  (|c| + 1) DBL_MIN on a leaf
        entry c exp(-t), DBL_MIN on a product or power.  (At ordinary magnitudes this term is 1e-308 and changes nothing.)
Operators propagate S to first order: S(a + b) = S(a) + S(b), S(a b) = S(a) |b| + |a| S(b), the product rule's da b + a db term by term,
S(a^e) = |e a^(e-1)| S(a).  Nothing in S is fitted to the device: it is derived here and validated against scikit-learn on the CPU
(tests/test_kernel_entries_cpu.py: e_ref <= REF_LIMIT eps on every case).

Bound (grad_truth's constants):  e(x) = max over entries |x - truth| / S;  e_dev <= BOUND max(e_ref, eps) with e_ref scikit-learn's error on
the same inputs, and e_ref <= REF_LIMIT eps."""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np

from grad_truth import BOUND, EPS, LD, REF_LIMIT, _require_extended      # noqa: F401  (re-exported: one set of constants)

DBL_MIN = float(np.finfo(np.float64).tiny)
LATTICE = 64.0                       # X = integers / 64
ONE_WORKGROUP = (1, 2, 15, 16, 17, 127, 128)
GENERAL = (129, 130, 191, 193, 257)


def _ns():
    from sklearn.gaussian_process.kernels import (RBF, DotProduct, Exponentiation, ExpSineSquared, Matern, RationalQuadratic, WhiteKernel,
                                                  ConstantKernel as C)
    return dict(RBF=RBF, Matern=Matern, W=WhiteKernel, C=C, RQ=RationalQuadratic, ESS=ExpSineSquared, Pow=Exponentiation, Dot=DotProduct,
                np=np, inf=np.inf)


# ---- designs ----------------------------------------------------------------------------------------------------------------------
def lattice_points(n, d, seed=0, span=140, dup=False):
    """n points of the lattice: d = 1: step * arange(n) / 64 with step = max(1, span // n) lattice steps, so that a few points still
    span about two units (arange(n) / 64 itself from n = span / 2 up); d > 1: integers in [0, span) / 64 per coordinate, drawn with a fixed
    seed.  ``dup``: rows 0 and n // 2 (and n - 1 and n // 3 where n > 4) coincide."""
    if d == 1:
        X = (np.arange(n, dtype=float) * max(1, span // max(n, 1)))[:, None] / LATTICE
    else:
        X = np.random.RandomState(1000 * d + n + seed).randint(0, span, size=(n, d)).astype(float) / LATTICE
    if dup and n >= 2:
        X[n // 2] = X[0]
        if n > 4:
            X[n - 1] = X[n // 3]
    return X


def two_scale_points(n):
    """A fine cluster (steps of 1 / 64) in the first half, the second half in steps of 1 / 4 beyond it (n = 127 ... 257: out to 16 ... 32
    units): with a length scale of 1 / 64 ... 1 / 2 the leaf derivatives run through the ordinary range, the subnormal band (exp argument
    -707.7 ... -745.2) and past it (exactly zero)."""
    h = n // 2
    a = np.arange(h, dtype=float) / LATTICE
    X = np.concatenate([a, a[-1] + 0.25 * np.arange(1, n - h + 1, dtype=float)])
    assert np.all(np.abs(X) < 64)
    return X[:, None]


def leaf_kernels(kernel):
    """The stationary leaves of a scikit-learn kernel, left to right."""
    from sklearn.gaussian_process.kernels import Exponentiation, Product, Sum
    if isinstance(kernel, (Sum, Product)):
        return leaf_kernels(kernel.k1) + leaf_kernels(kernel.k2)
    if isinstance(kernel, Exponentiation):
        return leaf_kernels(kernel.kernel)
    return [kernel] if hasattr(kernel, "length_scale") or hasattr(kernel, "sigma_0") else []


def _is_pow2(v):
    m, _ = np.frexp(np.asarray(v, dtype=float))
    return bool(np.all(m == 0.5))


def assert_exact_design(kernel, X):
    """X is on the lattice, every length scale is a power of two, and the float64 squared scaled distance of every pair -- in both device
    forms and in scikit-learn's -- equals the long-double one."""
    X = np.asarray(X, dtype=float)
    assert np.all(X * LATTICE == np.round(X * LATTICE)) and np.all(np.abs(X) < 64)
    for lf in leaf_kernels(kernel):
        if hasattr(lf, "sigma_0"):
            continue
        ls = np.broadcast_to(np.asarray(lf.length_scale, dtype=float), (X.shape[1],))
        assert _is_pow2(ls), lf
        if type(lf).__name__ in ("RationalQuadratic", "ExpSineSquared"):
            ls = np.ones(X.shape[1])                        # (these divide AFTER the distance: the sum is over unscaled differences)
        truth = (((X.astype(LD)[:, None, :] - X.astype(LD)[None, :, :]) / ls.astype(LD)) ** 2).sum(-1)
        form_a = np.zeros((len(X), len(X)))                 # (xi - xj) * inv_ls: the flattened gradient kernels
        form_b = np.zeros((len(X), len(X)))                 # xi / ls - xj / ls: the tree walk and the build (scikit-learn: pdist(X / ls))
        for m in range(X.shape[1]):
            u = (X[:, None, m] - X[None, :, m]) * (1.0 / ls[m])
            form_a = form_a + u * u
            w = X[:, None, m] / ls[m] - X[None, :, m] / ls[m]
            form_b = form_b + w * w
        assert np.array_equal(form_a.astype(LD), truth) and np.array_equal(form_b.astype(LD), truth), lf


# ---- truth ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Entries:
    v: np.ndarray           # (n, n) long double: the value
    Sv: np.ndarray
    d: list                 # P arrays (n, n): d / d log theta_p, scikit-learn's theta order
    Sd: list


def _pi():
    return LD(4) * np.arctan(LD(1))


def _exp_leaf(c, t):
    """g = c exp(-t) with its scale |g| (1 + |t|) + (|c| + 1) DBL_MIN."""
    g = c * np.exp(-t)
    return g, np.abs(g) * (1 + np.abs(t)) + (np.abs(c) + 1) * LD(DBL_MIN)


def _free(k, name):
    return not getattr(k, "hyperparameter_" + name).fixed


def _stationary(k, X, one_arg):
    from sklearn.gaussian_process.kernels import Matern
    n, d = X.shape
    ls = np.broadcast_to(np.asarray(k.length_scale, dtype=float), (d,)).astype(LD)
    D = ((X[:, None, :] - X[None, :, :]) / ls) ** 2          # (n, n, d), exact
    s = D.sum(-1)
    nu = float(k.nu) if isinstance(k, Matern) else np.inf
    aniso = np.ndim(k.length_scale) > 0 and np.size(k.length_scale) > 1
    dms = [D[:, :, m] for m in range(d)] if aniso else [s]
    one = np.ones_like(s)
    if nu == np.inf:
        t = s / 2
        v, Sv = _exp_leaf(one, t)
        ders = [_exp_leaf(dm, t) for dm in dms]
    elif nu == 0.5:
        t = np.sqrt(s)
        v, Sv = _exp_leaf(one, t)
        with np.errstate(divide="ignore", invalid="ignore"):
            ders = [_exp_leaf(np.where(t > 0, dm / np.where(t > 0, t, 1), LD(0)), t) for dm in dms]
    elif nu == 1.5:
        t = np.sqrt(3 * s)
        v, Sv = _exp_leaf(1 + t, t)
        ders = [_exp_leaf(3 * dm, t) for dm in dms]
    elif nu == 2.5:
        t = np.sqrt(5 * s)
        v, Sv = _exp_leaf(1 + t + t * t / 3, t)
        ders = [_exp_leaf(LD(5) / 3 * dm * (1 + t), t) for dm in dms]
    else:
        raise NotImplementedError(k)
    if one_arg:                                             # np.fill_diagonal(K, 1); every derivative is 0 there, exactly
        i = np.arange(n)
        v[i, i], Sv[i, i] = 1, 1
        for g, S in ders:
            g[i, i], S[i, i] = 0, 0
    if not _free(k, "length_scale"):
        ders = []
    return v, Sv, [g for g, _ in ders], [S for _, S in ders]


def _rq(k, X, one_arg):
    n = len(X)
    q = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    al, l2 = LD(k.alpha), LD(k.length_scale) ** 2
    u = q / (2 * al * l2)
    base = 1 + u
    v = np.exp(-al * np.log1p(u))
    ulp = (np.spacing((1.0 + u.astype(float))) / EPS).astype(LD)         # ulp(base) / eps: 1 in the first binade
    Sv = np.abs(v) + al * np.abs(v) / base * ulp + LD(DBL_MIN)
    g_l = q * v / (l2 * base)
    S_l = np.abs(g_l) + (al + 1) * np.abs(g_l) / base * ulp + LD(DBL_MIN)
    T1, T2 = al * np.log1p(u), q / (2 * l2 * base)
    T = al * (u / base - np.log1p(u))
    g_a = v * T
    S_a = np.abs(g_a) + (al * np.abs(v) * np.abs(T) / base + np.abs(v) * (al / base + T2 / base)) * ulp + np.abs(v) * (T1 + T2) + LD(DBL_MIN)
    if one_arg:
        i = np.arange(n)
        v[i, i], Sv[i, i] = 1, 1
        for a in (g_l, S_l, g_a, S_a):
            a[i, i] = 0
    d, Sd = [], []
    if _free(k, "alpha"):                                   # alphabetical: alpha, length_scale
        d.append(g_a), Sd.append(S_a)
    if _free(k, "length_scale"):
        d.append(g_l), Sd.append(S_l)
    return v, Sv, d, Sd


def _ess(k, X, one_arg):
    n = len(X)
    dist = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    l2, p = LD(k.length_scale) ** 2, LD(k.periodicity)
    a = _pi() * dist / p
    sn, cs = np.sin(a), np.cos(a)
    t = 2 * sn * sn / l2
    v = np.exp(-t)
    dv = -4 * sn * cs / l2 * v
    g_l = 4 / l2 * sn * sn * v
    g_p = 4 * a / l2 * cs * sn * v
    dg_l = 4 / l2 * (2 * sn * cs * v + sn * sn * dv)
    dg_p = 4 / l2 * ((cs * sn + a * (cs * cs - sn * sn)) * v + a * cs * sn * dv)
    tiny = LD(DBL_MIN)
    Sv = np.abs(v) * (1 + t) + np.abs(a * dv) + 2 * tiny
    S_l = np.abs(g_l) * (1 + t) + np.abs(a * dg_l) + LD(EPS) / 2 * a * a * (8 / l2 * cs * cs * v) + (4 / l2 + 1) * tiny
    S_p = np.abs(g_p) * (1 + t) + np.abs(a * dg_p) + (4 * np.abs(a) / l2 + 1) * tiny
    if one_arg:
        i = np.arange(n)
        v[i, i], Sv[i, i] = 1, 1
        for arr in (g_l, S_l, g_p, S_p):
            arr[i, i] = 0
    d, Sd = [], []
    if _free(k, "length_scale"):                            # alphabetical: length_scale, periodicity
        d.append(g_l), Sd.append(S_l)
    if _free(k, "periodicity"):
        d.append(g_p), Sd.append(S_p)
    return v, Sv, d, Sd


def _floor(S):
    """The underflow floor of a product or power: DBL_MIN on top of a scale, none where the scale is exactly zero (such an entry is a
    product with an exact zero and stays exact)."""
    return S + np.where(S > 0, LD(DBL_MIN), LD(0))


def _node(k, X, Y, one_arg):
    from sklearn.gaussian_process.kernels import (RBF, ConstantKernel, DotProduct, Exponentiation, ExpSineSquared, Product, RationalQuadratic,
                                                  Sum, WhiteKernel)
    shape = (len(X), len(Y))
    tiny = LD(DBL_MIN)
    if isinstance(k, (Sum, Product)):
        va, Sa, da, Sda = _node(k.k1, X, Y, one_arg)
        vb, Sb, db, Sdb = _node(k.k2, X, Y, one_arg)
        if isinstance(k, Sum):
            return va + vb, Sa + Sb, da + db, Sda + Sdb      # (the other side's derivative is zero: lists concatenate in theta order)
        aa, ab = np.abs(va), np.abs(vb)
        d = [g * vb for g in da] + [va * g for g in db]
        Sd = [_floor(S * ab + np.abs(g) * Sb) for g, S in zip(da, Sda)] + [_floor(Sa * np.abs(g) + aa * S) for g, S in zip(db, Sdb)]
        return va * vb, _floor(Sa * ab + aa * Sb), d, Sd
    if isinstance(k, Exponentiation):
        va, Sa, da, Sda = _node(k.kernel, X, Y, one_arg)
        e = LD(k.exponent)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = e * va ** (e - 1)
            f2 = np.abs(e * (e - 1)) * np.abs(va) ** (e - 2)
        return (va ** e, _floor(np.abs(f) * Sa), [g * f for g in da],
                [_floor(S * np.abs(f) + np.abs(g) * f2 * Sa) for g, S in zip(da, Sda)])
    if isinstance(k, WhiteKernel):
        w = LD(k.noise_level) * (np.eye(shape[0], dtype=LD) if one_arg else np.zeros(shape, LD))
        return w, np.abs(w), ([w.copy()] if _free(k, "noise_level") else []), ([np.abs(w)] if _free(k, "noise_level") else [])
    if isinstance(k, ConstantKernel):
        c = np.full(shape, LD(k.constant_value))
        return c, np.abs(c), ([c.copy()] if _free(k, "constant_value") else []), ([np.abs(c)] if _free(k, "constant_value") else [])
    if isinstance(k, DotProduct):
        s0 = LD(k.sigma_0) ** 2
        v = X @ Y.T + s0
        g = np.full(shape, 2 * s0)
        return v, np.abs(X) @ np.abs(Y).T + s0, ([g] if _free(k, "sigma_0") else []), ([np.abs(g)] if _free(k, "sigma_0") else [])
    assert one_arg, "the two-argument form is taken from the one-argument truth of the stacked points (cross_truth)"
    if isinstance(k, RationalQuadratic):
        return _rq(k, X, one_arg)
    if isinstance(k, ExpSineSquared):
        return _ess(k, X, one_arg)
    if isinstance(k, RBF):                                  # (Matern subclasses RBF)
        return _stationary(k, X, one_arg)
    raise NotImplementedError(k)


def entries_truth(kernel, X) -> Entries:
    """Value and every d / d log theta_p of the ONE-argument form kernel(X), entry by entry, in long double, with the scales."""
    _require_extended()
    Xl = np.asarray(X, dtype=np.float64).astype(LD)
    v, Sv, d, Sd = _node(kernel, Xl, Xl, True)
    assert len(d) == len(kernel.theta), (len(d), kernel)
    return Entries(v, Sv, d, Sd)


def cross_truth(kernel, X, Y):
    """Value of the TWO-argument form kernel(X, Y) with its scale: no diagonal rule, WhiteKernel off.  Leaves are evaluated on the stacked
    points [X; Y] with the diagonal rule off by construction: rows of X against rows of Y of a matrix whose diagonal is never read, except
    that a point of Y that equals a point of X meets it off the diagonal -- where exp(0) = 1 is the leaf's value anyway."""
    _require_extended()
    n = len(X)
    Z = np.concatenate([np.asarray(X, float), np.asarray(Y, float)]).astype(LD)
    v, Sv, _, _ = _node(_without_white(kernel), Z, Z, True)
    # the stacked one-argument form forces ITS diagonal to 1; block [0:n, n:] never touches that diagonal
    return v[:n, n:], Sv[:n, n:]


def _without_white(k):
    from sklearn.gaussian_process.kernels import ConstantKernel, Exponentiation, Product, Sum, WhiteKernel
    if isinstance(k, Sum):
        return Sum(_without_white(k.k1), _without_white(k.k2))
    if isinstance(k, Product):
        return Product(_without_white(k.k1), _without_white(k.k2))
    if isinstance(k, Exponentiation):
        return Exponentiation(_without_white(k.kernel), k.exponent)
    if isinstance(k, WhiteKernel):
        return ConstantKernel(0.0, "fixed")                 # kernel(X, Y): WhiteKernel contributes zeros (kernels.py WhiteKernel.__call__)
    return k


def entry_error(x, truth, S):
    """max over the entries of |x - truth| / S as a float; an entry whose scale is exactly zero must be exact; NaN / inf anywhere: inf."""
    x = np.asarray(x, dtype=np.float64)
    if not np.all(np.isfinite(x)):
        return float("inf")
    err = np.abs(x.astype(LD) - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(S > 0, err / np.where(S > 0, S, 1), np.where(err == 0, LD(0), LD(np.inf)))
    return float(np.max(e)) if e.size else 0.0


def reference_entries(kernel, X):
    """scikit-learn's float64 K and K_gradient (P, n, n) on the same inputs (its own 0 / 0 -> 0 at coincident points of Matern 1/2)."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        K, dK = kernel(np.asarray(X, dtype=float), eval_gradient=True)
    return K, np.ascontiguousarray(np.moveaxis(dK, 2, 0))


def value_claim(kernel):
    """What the header of csrc/kernels/build.hip.h claims for the VALUE entries against scikit-learn: "bits" (array_equal: the flattened
    family, and trees whose leaves are RBF / Matern under sums and products -- exp restated operation for operation),
    "ulps2" (a RationalQuadratic leaf alone: pow() against numpy's, an ulp or two), None (no claim: sin / cos of ExpSineSquared, pow() of an
    Exponentiation, RationalQuadratic under further operations, and DotProduct -- numpy's inner product sums in BLAS's order, and on this
    lattice every product and partial sum of xi . xj is exact, so equal bits here would say nothing about the order)."""
    from sklearn.gaussian_process.kernels import DotProduct, Exponentiation, ExpSineSquared, Product, RationalQuadratic, Sum
    if isinstance(kernel, RationalQuadratic):
        return "ulps2"

    def plain(k):
        if isinstance(k, (Sum, Product)):
            return plain(k.k1) and plain(k.k2)
        return not isinstance(k, (DotProduct, Exponentiation, ExpSineSquared, RationalQuadratic))

    return "bits" if plain(kernel) else None


def ulps_apart(a, b):
    """Largest distance in units of the last place between two float64 arrays of one sign pattern (finite, same shape)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all((a < 0) == (b < 0))
    return int(np.max(np.abs(a.view(np.int64) - b.view(np.int64)))) if a.size else 0


def within_bound(e_dev, e_ref):
    return e_dev <= BOUND * max(e_ref, EPS)


# ---- the case matrix ----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """``expr`` over the names of ``_ns``; ``design``: "lattice" (lattice_points) or "two_scale"; ``tree``: the descriptor is a postfix
    program (k_grad_small<true>, k_grad_contract<true, 1, true>), else the flattened family (<false>, <false, 2, true>)."""
    name: str
    n: int
    d: int
    expr: str
    tree: bool
    dup: bool = False
    design: str = "lattice"

    @property
    def id(self):
        return f"{self.name}-n{self.n}-d{self.d}"

    def kernel(self):
        return eval(self.expr, {"__builtins__": {}}, _ns())

    def X(self):
        if self.design == "two_scale":
            assert self.d == 1
            return two_scale_points(self.n)
        return lattice_points(self.n, self.d, dup=self.dup)


_W = " + W(0.5)"
_WF = " + W(0.5, noise_level_bounds='fixed')"
_L2, _L3 = "[0.5, 2.0]", "[0.5, 2.0, 0.25]"
_L8 = "[0.5, 2.0, 0.25, 4.0, 1.0, 8.0, 0.125, 16.0]"
# four anisotropic leaves at d = 2 with amplitudes: 4 amplitudes + 8 length scales = 12 parameters = GSUM_MAX_GRAD; every leaf has its own
# pair of length scales, so that a walk that reads another leaf's dimension, or leaf 0's for leaf 2, misses the truth in that parameter
FOUR_ANISO = ("C(1.25) * RBF([0.5, 2.0]) + C(0.75) * Matern([1.0, 0.25], nu=1.5) + C(1.5) * Matern([4.0, 0.5], nu=2.5)"
              " + C(0.5) * Matern([0.25, 1.0], nu=0.5)")

FLAT = [
    # (name, d, expr): RBF and Matern 1/2, 3/2, 5/2, with and without amplitude, additive constant, free / fixed white noise
    ("rbf", 1, "RBF(0.5)"),
    ("rbf-amp-w-add", 1, "C(1.25) * RBF(0.5)" + _W + " + C(0.25)"),
    ("m12-amp-wfix", 1, "C(0.75) * Matern(0.5, nu=0.5)" + _WF),
    ("m32-w", 1, "Matern(0.5, nu=1.5)" + _W),
    ("m52-amp-add", 1, "C(1.25) * Matern(0.5, nu=2.5) + C(0.25)"),
    ("m52-d2", 2, f"C(1.25) * Matern({_L2}, nu=2.5)" + _W),
    ("m32-d3", 3, f"C(1.25) * Matern({_L3}, nu=1.5)" + _WF + " + C(0.25)"),
    ("rbf-d8", 8, f"C(1.25) * RBF({_L8})" + _W),
    ("m12-d8", 8, f"Matern({_L8}, nu=0.5)" + _W),
]
TREES = [
    ("rq075", 1, "RQ(length_scale=0.5, alpha=0.75)"),
    ("rq48", 1, "RQ(length_scale=0.5, alpha=48.0)"),
    ("c-rq48", 1, "C(1.25) * RQ(length_scale=0.5, alpha=48.0)" + _W),
    ("ess13", 1, "ESS(length_scale=1.0, periodicity=3.0)"),
    ("c-ess", 1, "C(1.25) * ESS(length_scale=0.5, periodicity=0.75)" + _W),
    ("minf", 1, "Matern(0.5, nu=inf)"),
    ("c-minf-d2", 2, f"C(1.25) * Matern({_L2}, nu=inf)" + _W),
    ("c-dot", 2, "C(0.0625) * Dot(sigma_0=0.5) + RBF(1.0)" + _W),
    ("pow2", 1, "Pow(C(1.25) * RQ(length_scale=0.5, alpha=0.75) + C(0.5), 2)" + _W),
    ("pow3", 1, "Pow(Matern(1.0, nu=1.5) + C(0.25), 3)" + _W),
    ("product", 2, f"RQ(length_scale=1.0, alpha=0.75) * RBF({_L2}) + C(0.25)" + _W),
    ("sum-of-products", 1, "C(1.25) * RBF(0.5) * Matern(2.0, nu=2.5) + C(0.75) * Matern(0.5, nu=0.5) * ESS(length_scale=1.0, periodicity=3.0)"
                           + _W),
    ("rbf+rbf", 1, "C(1.25) * RBF(0.5) + C(0.5) * Matern(2.0, nu=1.5)"),
    ("four-aniso", 2, FOUR_ANISO),
]


def _spread(specs, orders, tree):
    """Every kernel at two orders, every order under some kernel: kernel i takes orders i and i + 3 (mod the list) of the path."""
    out = []
    for i, (name, d, expr) in enumerate(specs):
        for n in sorted({orders[i % len(orders)], orders[(i + 3) % len(orders)]}):
            out.append(Case(name, n, d, expr, tree, dup=("nu=0.5" in expr and n >= 2)))
    return out


CASES = (_spread(FLAT, ONE_WORKGROUP, False) + _spread(FLAT, GENERAL, False)
         + _spread(TREES, ONE_WORKGROUP, True) + _spread(TREES, GENERAL, True))
# orders that no kernel of the spread reached get the first kernel of the family
for _orders, _specs, _tree in ((ONE_WORKGROUP, FLAT, False), (GENERAL, FLAT, False), (ONE_WORKGROUP, TREES, True), (GENERAL, TREES, True)):
    for _n in _orders:
        if not any(c.n == _n and c.tree == _tree for c in CASES):
            CASES.append(Case(_specs[1][0], _n, _specs[1][1], _specs[1][2], _tree))

# the two-argument form kernel(X, Y): EVERY tree kernel, at its first one-workgroup order and its first general-path order
TWO_ARG_CASES = [next(c for c in CASES if c.tree and c.name == name and (c.n <= 128) == small)
                 for name, _, _ in TREES for small in (True, False)]
TWO_ARG_M = (1, 127, 129)

# the two-scale design: leaf derivatives in the subnormal band and past -745.2
TWO_SCALE = [
    Case("far-rbf", 193, 1, "C(1.25) * RBF(0.5)" + _W, False, design="two_scale"),
    Case("far-m52", 257, 1, "Matern(0.0625, nu=2.5)" + _W, False, design="two_scale"),
    Case("far-m32", 128, 1, "C(1.25) * Matern(0.03125, nu=1.5)", False, design="two_scale"),
    Case("far-m12", 130, 1, "Matern(0.015625, nu=0.5)" + _W, False, design="two_scale"),
    Case("far-minf", 127, 1, "C(1.25) * Matern(0.25, nu=inf)" + _W, True, design="two_scale"),
    Case("far-ess", 191, 1, "C(1.25) * ESS(length_scale=0.03125, periodicity=48.0)" + _W, True, design="two_scale"),
]
ALL_CASES = CASES + TWO_SCALE
CASE_IDS = [c.id for c in ALL_CASES]

_TRUTHS = {}


def case_truth(case: Case):
    """(kernel, X, Entries, K_ref, dK_ref (P, n, n)) of a case: one truth evaluation per session, read-only."""
    if case.id not in _TRUTHS:
        kern, X = case.kernel(), case.X()
        T = entries_truth(kern, X)
        K, dK = reference_entries(kern, X)
        for a in (X, K, dK):
            a.setflags(write=False)
        _TRUTHS[case.id] = (kern, X, T, K, dK)
    return _TRUTHS[case.id]


def leaf_parameters(T: Entries, far):
    """The parameters whose derivative carries the leaf's exponential as a factor (length scales, periodicity, amplitude): on the far
    entries their truth is a modest multiple of exp(-745.3) = 2^-1075, where an additive constant's or the white noise's is its weight.
    In float64 the exponential is exactly 0.0 there and so is the entry."""
    return [p for p in range(len(T.d)) if far.any() and np.all(np.abs(T.d[p][far]) < LD(2.0) ** -1040)]


def far_mask(case: Case, X):
    """Off-diagonal entries of a single-leaf case whose exp argument lies beyond -745.2 (exactly zero in float64), and the ones in the
    subnormal band (-745.2 ... -708.4)."""
    t = exp_argument(case, X)
    return t > LD(745.3), (t > LD(708.4)) & (t < LD(745.1))


def table_range(case: Case, X):
    """Entries whose exponential the device takes from its restatement of numpy's table algorithm (|argument| < 707.7) or knows to be
    exactly zero: where the header of build.hip.h claims scikit-learn's bits.  In between (results below 4.6e-308) the device library's
    exp and numpy's scalar path may round a subnormal differently (tests/build_classes.py pins that band for the flattened family)."""
    t = exp_argument(case, X)
    return (t < LD(707.5)) | (t > LD(745.5))


def exp_argument(case: Case, X):
    """-(the exp argument) of every entry of a single-leaf case, in long double."""
    from sklearn.gaussian_process.kernels import ExpSineSquared, Matern
    lf = leaf_kernels(case.kernel())
    assert len(lf) == 1
    lf = lf[0]
    Xl = np.asarray(X, float).astype(LD)
    dist = np.abs(Xl - Xl.T)
    if isinstance(lf, ExpSineSquared):
        t = 2 * (np.sin(_pi() * dist / LD(lf.periodicity)) / LD(lf.length_scale)) ** 2
    else:
        r = dist / LD(lf.length_scale)
        nu = float(lf.nu) if isinstance(lf, Matern) else np.inf
        t = {np.inf: r * r / 2, 0.5: r, 1.5: np.sqrt(LD(3)) * r, 2.5: np.sqrt(LD(5)) * r}[nu]
    return t
