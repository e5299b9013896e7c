"""Shared cases of the Toeplitz gradient pieces (test_toeplitz_grad_cpu.py on backend='cpu', test_gpu_toeplitz_grad.py on 'hip'):
``toeplitz_inverse_column``, ``toeplitz_solve``, ``toeplitz_grad`` and the model layer on top.

The yardstick is toeplitz_cases._rule: against a truth the device is at most 4 x the cpu backend's distance, with the floor 64 * 2^-53
relative to the largest magnitude of the quantity; on the ill-conditioned goldens also at most the distance of numpy's dense fp64
route.  The cpu backend itself is held to the floor on the well-conditioned ARFIMA columns and to numpy's dense route on the goldens,
as section 18 holds it.  Every check takes the backend and returns what it measured."""
import functools
import json
import os

import numpy as np
from scipy.linalg import cho_factor, cho_solve, toeplitz

import gsum_amd as gm
import toeplitz_cases as tc
from toeplitz_cases import EPS, FLOOR, LD, _rule

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toeplitz_grad.json")


def cols_at(n):
    """Four right-hand sides (ones, alternating signs, a ramp, normals); two from n = 4095 up, where the cpu yardstick is the cost."""
    return 4 if n < 4095 else 2


def rel(a, b, scale=None):
    """max |a - b| / max |scale or b| in long double, as a float."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    s = np.max(np.abs(b if scale is None else np.asarray(scale, dtype=LD)))
    return float(np.max(np.abs(a - b)) / s) if s > 0 else float(np.max(np.abs(a - b)))


# ---- (1), (2): exact identities and the closed-form inverse column on ARFIMA(0, d, 0) -------------------------------------------------

def arfima_inverse_column(n, d):
    """x = T^-1 e_0 of the ARFIMA column with t_0 = 1 in long double: with k = n - 1 and gamma_j = d / (j - d),
    x = (1, -phi_k1, .., -phi_kk) / prod_{j <= k} (1 - gamma_j^2), phi_k1 = k d / (k - d), phi_k,j+1 = phi_kj (k - j) / (j + 1) * (j - d)
    / (k - d - j)."""
    k, dl = n - 1, LD(d)
    x = np.zeros(n, dtype=LD)
    x[0] = 1
    if k >= 1:
        phi = LD(k) * dl / (k - dl)
        x[1] = -phi
        for j in range(1, k):
            phi = phi * LD(k - j) / LD(j + 1) * (j - dl) / (k - dl - j)
            x[j + 1] = -phi
    return x / tc.arfima_energies(n, d)[-1]


def toeplitz_times_ld(t, A, absolute=False):
    """T A (or |T| |A|) in long double for the symmetric Toeplitz matrix of the first column t and the columns A (n, c)."""
    t = np.asarray(t, dtype=LD)
    A = np.asarray(A, dtype=LD)
    if absolute:
        t, A = np.abs(t), np.abs(A)
    n = len(t)
    out = np.empty_like(A)
    for c in range(A.shape[1]):
        a = A[:, c]
        out[:, c] = np.convolve(t, a)[:n] + np.convolve(t, a[::-1])[:n][::-1] - t[0] * a
    return out


@functools.lru_cache(maxsize=None)
def _identity_inputs(n):
    """(ds, t (m, n), dt (m, 2, n) = [t, e_0] per first column, Z (n, cols_at(n))): made once, never written to.  d runs over DS: both
    in one call below n = 4095, from there on one per size, alternating with the size, so that the cpu yardstick stays within seconds."""
    ds = tc.DS if n < 4095 else (tc.DS[tc.SIZES.index(n) % 2],)
    t = np.stack([tc.arfima_column(n, d) for d in ds])
    e0 = np.zeros(n)
    e0[0] = 1.0
    dt = np.stack([np.stack([ti, e0]) for ti in t])
    Z = tc.rhs_columns(n, cols_at(n))
    for a in (t, dt, Z):
        a.setflags(write=False)
    return ds, t, dt, Z


@functools.lru_cache(maxsize=None)
def identity_distances(backend, n):
    """The distances of a backend from the exact identities of the pair dt = [t, e_0] and from the closed-form x, the worst over the
    two first columns: trace(t) = n, H(t) = G, trace(e_0) = sum_m (n - 2 m) x_m^2 / x_0 on the closed-form x, H(e_0) = alpha^T alpha
    (the backend's own alpha, in long double), T alpha = Z (long double, relative to max |T| |alpha|: what rounding alpha to fp64
    alone moves the product by) and x itself."""
    ds, t, dt, Z = _identity_inputs(n)
    m = len(ds)
    G, sld, info, trace, H = gm.toeplitz_grad(t, dt, Z, backend=backend)
    x, info_x = gm.toeplitz_inverse_column(t, backend=backend)
    alpha, info_a = gm.toeplitz_solve(t, Z, backend=backend)
    c = Z.shape[1]
    assert G.shape == (m, 1, c, c) and trace.shape == (m, 2) and H.shape == (m, 1, 2, c, c) and x.shape == (m, n) and alpha.shape == (m, n, c)
    assert not info.any() and not info_x.any() and not info_a.any(), (info, info_x, info_a)
    assert np.array_equal(H, H.transpose(0, 1, 2, 4, 3))
    if backend != "cpu" or n < 4095:                                    # on the cpu backend G is _cpu_gram's by construction: seconds saved
        Gv, sv, iv = gm.toeplitz_gram(t, Z, backend=backend)
        assert np.array_equal(G, Gv) and np.array_equal(sld, sv) and np.array_equal(info, iv)
    out = dict(trace_t=0.0, H_t=0.0, trace_e0=0.0, H_e0=0.0, residual=0.0, x=0.0)
    k = np.arange(n, dtype=LD)
    for i, d in enumerate(ds):
        xt = arfima_inverse_column(n, d)
        al = alpha[i].astype(LD)
        got = dict(trace_t=abs(trace[i, 0] - n) / n, H_t=rel(H[i, 0, 0], G[i, 0]), trace_e0=rel(trace[i, 1], np.sum((n - 2 * k) * xt * xt) / xt[0]),
                   H_e0=rel(H[i, 0, 1], al.T @ al), residual=rel(toeplitz_times_ld(t[i], al), Z, toeplitz_times_ld(t[i], al, absolute=True)),
                   x=rel(x[i], xt))
        out = {key: max(out[key], float(got[key])) for key in out}
    return out


def check_identities(backend, n):
    """(1), (2): under the rule against the cpu backend's own distances; the cpu backend itself within the floor."""
    got, cpu = identity_distances(backend, n), identity_distances("cpu", n)
    print(f"toeplitz grad identities {backend} n={n}: " + ", ".join(f"{k} {got[k] / EPS:.2f} (cpu {cpu[k] / EPS:.2f})" for k in got))
    for k in got:
        assert cpu[k] <= FLOOR, (n, k, cpu[k])
        assert got[k] <= _rule(cpu[k]), (n, k, got[k], cpu[k])
    return {k: v / EPS for k, v in got.items()}


# ---- (3): goldens against mpmath ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def golden_arrays():
    """The long vectors of the goldens, toeplitz_grad.npz: "<name>/dt" (n,) and "<name>/alpha" (n, cols), float64."""
    with np.load(GOLDEN[:-5] + ".npz") as f:
        return {k: f[k] for k in f.files}


def golden_names():
    return [c["name"] for c in golden()["cases"]]


def grad_distances(trace, H, alpha, case):
    """(trace, H, alpha) distances from a golden: |trace error| / |trace|, entrywise maxima relative to max |H| and max |alpha|."""
    return (float(abs(trace - case["trace"]) / abs(case["trace"])), rel(H, np.array(case["H"])), rel(alpha, golden_arrays()[case["name"] + "/alpha"]))


@functools.lru_cache(maxsize=None)
def _golden_yardsticks(name):
    """(t, dt (1, n), Z, case, distances of numpy's dense fp64 route on the same T, distances of the cpu backend)."""
    case = [c for c in golden()["cases"] if c["name"] == name][0]
    t = tc.hex_column([c for c in tc.ill_cases() if c["name"] == name][0])
    dt = golden_arrays()[name + "/dt"][None]
    Z = tc.rhs_columns(case["n"], case["cols"])
    cf = cho_factor(toeplitz(t), lower=True)
    Ti = cho_solve(cf, np.eye(len(t)))
    V = cho_solve(cf, Z)
    dT = toeplitz(dt[0])
    d_np = grad_distances(float(np.einsum("ij,ij->", Ti, dT)), np.einsum("ia,ij,jb->ab", V, dT, V), V, case)
    return t, dt, Z, case, d_np, _backend_distances("cpu", t, dt, Z, case)


def _backend_distances(backend, t, dt, Z, case):
    G, sld, info, trace, H = gm.toeplitz_grad(t, dt, Z, backend=backend)
    alpha, info_a = gm.toeplitz_solve(t, Z, backend=backend)
    assert info == 0 and info_a == 0
    return grad_distances(trace[0], H[0, 0], alpha, case)


def check_golden(backend, name):
    """(3): trace, H and alpha against the mpmath truth: at most numpy's dense route's distance on the same T (with the floor), and
    within 4 x the cpu backend's."""
    t, dt, Z, case, d_np, d_cpu = _golden_yardsticks(name)
    d = d_cpu if backend == "cpu" else _backend_distances(backend, t, dt, Z, case)
    names = ("trace", "H", "alpha")
    print(f"toeplitz grad golden {name} {backend}: " + ", ".join(f"{names[k]} {d[k]:.3g} (numpy {d_np[k]:.3g}, cpu {d_cpu[k]:.3g})" for k in range(3)))
    for k in range(3):
        assert d[k] <= max(d_np[k], FLOOR), (name, names[k], d, d_np)
        assert d[k] <= 4 * max(d_cpu[k], FLOOR), (name, names[k], d, d_cpu)
    return d, d_np, d_cpu


def check_golden_extended(backend, name):
    """(3), sharper and for the device alone.  It carries the recursion, x and every sum in double-double, 106 bits, where the cpu
    backend has long double's 64: a unit roundoff 2^42 times smaller.  On the ill-conditioned goldens the cpu backend's distance is set
    by that width, so the device's trace and alpha -- each rounded to fp64 once, at the end -- are held to 2^-20 of the cpu backend's
    distance (half of the 42 bits is left as margin), floor 64 * 2^-53.  H is held to the cpu backend's distance itself: alpha is
    rounded to fp64 before the contraction, and that rounding reaches H amplified by the cancellation in alpha^T dT alpha, which a
    floor relative to max|H| does not cover.  The rule's 4 x max(cpu, floor) and numpy's dense route are thousands of times wider than
    the device's own error here and do not see a low word that is lost (mutations)."""
    t, dt, Z, case, d_np, d_cpu = _golden_yardsticks(name)
    d = _backend_distances(backend, t, dt, Z, case)
    for k, what in enumerate(("trace", "H", "alpha")):
        bound = max(d_cpu[k] * (1.0 if what == "H" else 2.0 ** -20), FLOOR)
        assert d[k] <= bound, (name, what, d, d_cpu, bound)
    return d


# ---- (4): properties and refusals ----------------------------------------------------------------------------------------------------------

def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def check_properties(backend, n=257):
    """(4): bitwise reproducibility; independence of m, of the other sets, of their order and of the column chunking; H bitwise
    symmetric; G, sum_log_diag and info those of toeplitz_gram."""
    rng = np.random.RandomState(3)
    t1 = tc.kms_column(n, 0.5) + 0.25 * tc.kms_column(n, -0.5)
    dt1 = np.stack([np.arange(n) * t1, np.cos(0.1 * np.arange(n))])
    c = 5
    Zs = rng.randn(12, n, c)                                            # 12 sets

    def flat(sets):
        return sets.transpose(1, 0, 2).reshape(n, -1)

    one = gm.toeplitz_grad(t1, dt1, flat(Zs[:1]), 1, backend=backend)
    assert one[2] == 0 and _same(one, gm.toeplitz_grad(t1, dt1, flat(Zs[:1]), 1, backend=backend))                # two runs
    assert np.array_equal(one[4], one[4].transpose(0, 1, 3, 2))
    assert _same(one[:3], gm.toeplitz_gram(t1, flat(Zs[:1]), 1, backend=backend))
    many = np.stack([tc.kms_column(n, 0.9 * np.cos(i)) for i in range(33)])
    many[20] = t1
    dmany = np.stack([np.stack([np.sin(i + np.arange(n)), many[i]]) for i in range(33)])
    dmany[20] = dt1
    got = gm.toeplitz_grad(many, dmany, flat(Zs[:1]), 1, backend=backend)
    assert not got[2].any() and _same([g[20] for g in got], one)                                                   # alone and among 33
    sets = gm.toeplitz_grad(t1, dt1, flat(Zs), 12, backend=backend)
    assert np.array_equal(sets[0][0], one[0][0]) and np.array_equal(sets[4][0], one[4][0]) and np.array_equal(sets[3], one[3])
    rev = gm.toeplitz_grad(t1, dt1, flat(Zs[::-1]), 12, backend=backend)
    assert np.array_equal(rev[0][::-1], sets[0]) and np.array_equal(rev[4][::-1], sets[4])                         # the sets reversed
    Z16 = rng.randn(n, 16)
    full = gm.toeplitz_grad(t1, dt1, Z16, 1, backend=backend)
    a16, _ = gm.toeplitz_solve(t1, Z16, backend=backend)
    for lo, hi in ((0, 5), (5, 10), (10, 16)):                                                                     # c = 16 at once and in three calls
        part = gm.toeplitz_grad(t1, dt1, Z16[:, lo:hi], 1, backend=backend)
        assert np.array_equal(part[0][0], full[0][0][lo:hi, lo:hi]) and np.array_equal(part[4][0], full[4][0][:, lo:hi, lo:hi])
        assert part[1] == full[1] and np.array_equal(part[3], full[3])
        assert np.array_equal(gm.toeplitz_solve(t1, Z16[:, lo:hi], backend=backend)[0], a16[:, lo:hi])
    x1, _ = gm.toeplitz_inverse_column(t1, backend=backend)
    xm, _ = gm.toeplitz_inverse_column(many, backend=backend)
    assert np.array_equal(xm[20], x1)
    # scaling a column of Z by a power of two scales alpha, and H with it, exactly
    s = np.array([2.0 ** 40, 2.0 ** -30, 1.0, 2.0 ** 7, 0.5])
    sc = gm.toeplitz_grad(t1, dt1, flat(Zs[:1]) * s, 1, backend=backend)
    if backend != "cpu":
        assert np.array_equal(sc[4][0], one[4][0] * np.outer(s, s)) and np.array_equal(sc[0][0], one[0][0] * np.outer(s, s))


def check_failure_between_good(backend, n=513, d=0.25):
    """(4): a first column that fails at step p + 1 (built as toeplitz_cases.check_late_failures builds it, p at a thread boundary of
    the class) between two good ones: its outputs are NaN, the good ones bit for bit what they are alone."""
    E = tc.elements_per_thread(n)
    p = ((n // E) // 2) * E
    goods = [tc.arfima_column(n, d), tc.arfima_column(n, tc.DS[1])]
    bad = goods[0].copy()
    bad[p] += 1.5 * float(tc.arfima_energies(n, d)[p - 1])
    Z = tc.rhs_columns(n, 2)
    ts = np.stack([goods[0], bad, goods[1]])
    dts = np.stack([np.stack([t, np.cos(np.arange(n))]) for t in ts])
    got = gm.toeplitz_grad(ts, dts, Z, backend=backend)
    assert list(got[2]) == [0, p + 1, 0], got[2]
    assert all(np.isnan(g[1]).all() for g in (got[0], got[1], got[3], got[4]))
    x, ix = gm.toeplitz_inverse_column(ts, backend=backend)
    al, ia = gm.toeplitz_solve(ts, Z, backend=backend)
    assert list(ix) == [0, p + 1, 0] and list(ia) == [0, p + 1, 0] and np.isnan(x[1]).all() and np.isnan(al[1]).all()
    for i in (0, 2):
        alone = gm.toeplitz_grad(ts[i], dts[i], Z, backend=backend)
        assert alone[2] == 0 and _same([g[i] for g in got], alone), i
        assert np.array_equal(x[i], gm.toeplitz_inverse_column(ts[i], backend=backend)[0])
        assert np.array_equal(al[i], gm.toeplitz_solve(ts[i], Z, backend=backend)[0])
        assert np.isfinite(got[3][i]).all() and np.isfinite(got[4][i]).all()
    return [int(v) for v in got[2]]


CHUNKED = dict(n=513, c=16, n_sets=1023, m=3)


def check_chunk_loop(backend):
    """(4): toeplitz_cases.check_chunk_loop for ``toeplitz_grad`` and ``toeplitz_solve``, whose launches keep Y and alpha of a first
    column in flight together: half the budget each.  n * ncols = 8 396 784 exceeds 2^28 / 32, so the three first columns go through one
    per launch (offsets into t, dt, sum_log_diag, info, G, H, trace and alpha; the scratch reused), and one set fewer would take two:
    the smallest such shape at c = 16 and an odd n above a class boundary.  P = 1.  The middle first column fails at step 3 and is NaN
    throughout.  For each good one G, H and sum_log_diag of the first, middle and last set, and trace, are bitwise those of a call with
    that column and those three sets alone, and alpha at their 48 columns bitwise that of such a call.  Device only (67 MB of Z, 200 MB
    of alpha back): 0.4 s measured on an MI355X."""
    n, c, n_sets, m = (CHUNKED[k] for k in ("n", "c", "n_sets", "m"))
    half = tc.Y_BUDGET // 2
    assert n * n_sets * c == 8396784 > 2 ** 28 // 32
    assert tc.first_columns_per_launch(n, n_sets * c, m, half) == 1 and tc.first_columns_per_launch(n, (n_sets - 1) * c, m, half) == 2
    goods = [tc.arfima_column(n, d) for d in tc.DS]
    bad = goods[0].copy()
    p = 2
    bad[p] += 1.5 * float(tc.arfima_energies(n, tc.DS[0])[p - 1])
    Z = np.asfortranarray(np.random.RandomState(11).standard_normal((n_sets * c, n)).T)
    ts = np.stack([goods[0], bad, goods[1]])
    dts = np.stack([np.cos(np.arange(n))[None]] * m)
    got = gm.toeplitz_grad(ts, dts, Z, n_sets, backend=backend)
    assert list(got[2]) == [0, p + 1, 0], got[2]
    assert all(np.isnan(g[1]).all() for g in (got[0], got[1], got[3], got[4]))
    al, ia = gm.toeplitz_solve(ts, Z, backend=backend)
    assert list(ia) == [0, p + 1, 0] and np.isnan(al[1]).all()
    pick = [0, n_sets // 2, n_sets - 1]
    cols3 = np.concatenate([np.arange(s * c, (s + 1) * c) for s in pick])
    Z3 = Z[:, cols3]
    for i in (0, 2):
        G1, s1, i1, tr1, H1 = gm.toeplitz_grad(ts[i], dts[i], Z3, 3, backend=backend)
        assert i1 == 0 and np.array_equal(got[0][i][pick], G1) and np.array_equal(got[4][i][pick], H1), i
        assert got[1][i] == s1 and np.array_equal(got[3][i], tr1), i
        a1, j1 = gm.toeplitz_solve(ts[i], Z3, backend=backend)
        assert j1 == 0 and np.array_equal(al[i][:, cols3], a1), i
        assert np.isfinite(got[0][i]).all() and np.isfinite(got[4][i]).all() and np.isfinite(got[3][i]).all() and np.isfinite(a1).all()
    return [int(v) for v in got[2]]


def check_shape_refusals(backend):
    """(4): the shapes the Python layer refuses, on either backend."""
    import pytest
    t, Z = tc.kms_column(8, 0.5), np.ones((8, 2))
    dt = np.stack([t, t])
    with pytest.raises(ValueError, match="P >= 1"):
        gm.toeplitz_grad(t, np.zeros((0, 8)), Z, backend=backend)
    with pytest.raises(ValueError, match="dt must have shape"):
        gm.toeplitz_grad(t, np.ones((2, 7)), Z, backend=backend)
    with pytest.raises(ValueError, match="dt must have shape"):
        gm.toeplitz_grad(np.stack([t, t]), dt, Z, backend=backend)               # (m, n) first columns need (m, P, n)
    with pytest.raises(ValueError, match="n_sets"):
        gm.toeplitz_grad(t, dt, np.ones((8, 5)), n_sets=2, backend=backend)
    with pytest.raises(ValueError, match="at most 16"):
        gm.toeplitz_grad(t, dt, np.ones((8, 17)), backend=backend)
    with pytest.raises(ValueError, match="Z must have shape"):
        gm.toeplitz_solve(t, np.ones((7, 2)), backend=backend)
    with pytest.raises(ValueError, match="t must have shape"):
        gm.toeplitz_inverse_column(np.ones((2, 2, 2)), backend=backend)


# ---- (6): the model layer ------------------------------------------------------------------------------------------------------------------

def model_process(cls, backend, **kw):
    """toeplitz test_toeplitz_cpu._process with the length scale freed: Matern-1/2 plus a fixed WhiteKernel, well conditioned."""
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    return cls(kernel=Matern(0.2, nu=0.5) + WhiteKernel(1e-6, noise_level_bounds="fixed"), backend=backend, **kw)


MODEL_CLASSES = (("gaussian", dict(center=0.1, disp=1.5, df=2, scale=0.7)), ("student", dict(df=3, scale=0.9)))
MODEL_THETAS = (np.log([0.05]), np.log([0.1]), np.log([0.15]))


def model_class(name):
    return gm.ConjugateGaussianProcess if name == "gaussian" else gm.ConjugateStudentProcess


def model_xy(n, r=3):
    return np.linspace(0, 1, n)[:, None], np.random.RandomState(1).randn(n, r)


def check_model_gradient(backend, name, n):
    """(6): the structured batch's (lml, grad) against a long-double truth: grad_truth.pieces_truth on the exact Toeplitz matrix of
    the route's own first column and derivative column, pushed through the class's host algebra.  The structured route is no farther
    from it than 4 x the dense route, floor 64 * 2^-53 max|grad|.  Values bit-equal to the route without the gradient; every entry of
    the batch equals the batch of one."""
    import grad_truth
    from gsum_amd.conjugate import lml_grad_from_gram, student_lml_grad_from_gram
    kw = dict(MODEL_CLASSES)[name]
    gp = model_process(model_class(name), backend, optimizer=None, **kw)
    X, y = model_xy(n)
    thetas = list(MODEL_THETAS)
    got = gp.log_marginal_likelihood_batch(thetas, X=X, y=y, structure="toeplitz", eval_gradient=True)
    vals = gp.log_marginal_likelihood_batch(thetas, X=X, y=y, structure="toeplitz")
    assert isinstance(got, list) and [type(g) for g in got] == [tuple] * 3 and all(g[1].shape == (1,) for g in got)
    assert [g[0] for g in got] == list(vals)
    worst = 0.0
    Z = gp._rhs(X, y)
    for k, (th, g) in enumerate(zip(thetas, got)):
        alone = gp.log_marginal_likelihood_batch([th], X=X, y=y, structure="toeplitz", eval_gradient=True)[0]
        assert alone[0] == g[0] and np.array_equal(alone[1], g[1])
        if n > 100 and k != 1:                                          # the long-double Cholesky is O(n^3): one theta at the larger size
            continue
        t = gm.toeplitz_column(gp.kernel.clone_with_theta(th), X, gp.nugget, backend=backend)
        dt = gm.toeplitz_gradient_columns(gp.kernel, X, th)
        T = grad_truth.pieces_truth(toeplitz(t), np.stack([toeplitz(d) for d in dt], axis=2))
        r = grad_truth.add_rhs(T, "z", Z)
        fn = lml_grad_from_gram if name == "gaussian" else student_lml_grad_from_gram
        prior = (gp.center0, gp.disp0, gp.df0, gp.scale0)
        lml_t, grad_t = fn(r.G.astype(float), float(T.sld), T.trace.astype(float), r.H.astype(float), n, *prior)
        dense = gp.log_marginal_likelihood(th, eval_gradient=True, X=X, y=y)
        floor = FLOOR * float(np.max(np.abs(grad_t)))
        d_s, d_d = float(np.max(np.abs(g[1] - grad_t))), float(np.max(np.abs(dense[1] - grad_t)))
        print(f"toeplitz grad model {backend} {name} n={n} theta={th[0]:.3f}: structured {d_s:.3g}, dense {d_d:.3g}, floor {floor:.3g}; "
              f"lml {abs(g[0] - lml_t) / abs(lml_t):.3g}")
        assert d_s <= max(4 * d_d, floor), (name, th, d_s, d_d, floor)
        assert abs(g[0] - lml_t) <= 1e-12 * abs(lml_t)
        worst = max(worst, d_s / float(np.max(np.abs(grad_t))))
    return worst


class Counters:
    """Counts the calls of the structured and of the dense likelihood evaluators while a fit runs (monkeypatch)."""

    def __init__(self, monkeypatch, gp):
        from gsum_amd import toeplitz as tz
        self.structured = self.dense = 0
        for name in ("toeplitz_grad", "toeplitz_gram"):
            monkeypatch.setattr(tz, name, self._wrap(getattr(tz, name), "structured"))
        ctx = gp._context()
        for name in ("lml_grad", "lml_grad_batch", "lml_batch"):
            monkeypatch.setattr(ctx, name, self._wrap(getattr(ctx, name), "dense"), raising=True)

    def _wrap(self, fn, which):
        def counted(*a, **k):
            setattr(self, which, getattr(self, which) + 1)
            return fn(*a, **k)
        return counted


FACTR_EPS = 1e7 * np.finfo(float).eps                                  # L-BFGS stops on a relative decrease of factr * eps = 2.2e-9


def check_fit(backend, name, n, monkeypatch):
    """(6): fit(structure="toeplitz") sends every calibration evaluation down the structured route and ends within 100 factr eps
    |value| of the dense fit's optimum; the lock-step restarts give the sequential loop's optimum; fit(structure=None) never touches
    the structured route and equals fit()."""
    cls, kw = model_class(name), dict(MODEL_CLASSES)[name]
    X, y = model_xy(n)
    dense = model_process(cls, backend, **kw).fit(X, y)
    gp = model_process(cls, backend, **kw)
    with monkeypatch.context() as mpc:
        cnt = Counters(mpc, gp)
        gp.fit(X, y, structure="toeplitz")
        assert cnt.structured > 0 and cnt.dense == 0, (cnt.structured, cnt.dense)
        evaluations = cnt.structured
    v_s, v_d = gp.log_marginal_likelihood_value_, dense.log_marginal_likelihood_value_
    diff = abs(v_s - v_d) / abs(v_d)
    print(f"toeplitz fit {backend} {name} n={n}: structured {v_s!r} dense {v_d!r} relative difference {diff:.3g} in {evaluations} evaluations")
    assert diff <= 100 * FACTR_EPS, (v_s, v_d)
    assert gp._fit_structure is None
    # predict after a structured fit is the dense code on the fitted kernel
    Xs = np.linspace(0.05, 0.95, 7)[:, None]
    same = cls(kernel=gp.kernel_, backend=backend, optimizer=None, **kw).fit(X, y)
    assert np.array_equal(gp.predict(Xs), same.predict(Xs))
    # the restarts: lock step against the sequential loop, both structured
    fits = []
    for lockstep in (True, False):
        g = model_process(cls, backend, n_restarts_optimizer=2, random_state=5, **kw)
        g.batch_restarts = lockstep
        with monkeypatch.context() as mpc:
            cnt = Counters(mpc, g)
            g.fit(X, y, structure="toeplitz")
            assert cnt.structured > 0 and cnt.dense == 0, (lockstep, cnt.structured, cnt.dense)
        fits.append(g)
    assert np.array_equal(fits[0].kernel_.theta, fits[1].kernel_.theta)
    assert fits[0].log_marginal_likelihood_value_ == fits[1].log_marginal_likelihood_value_
    # structure=None: today's path
    g = model_process(cls, backend, **kw)
    with monkeypatch.context() as mpc:
        cnt = Counters(mpc, g)
        g.fit(X, y, structure=None)
        assert cnt.structured == 0 and cnt.dense > 0
    assert np.array_equal(g.kernel_.theta, dense.kernel_.theta) and g.log_marginal_likelihood_value_ == v_d
    return diff
