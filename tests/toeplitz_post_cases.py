"""Shared cases of the posterior pieces of the Toeplitz path (test_toeplitz_post_cpu.py on backend='cpu', test_gpu_toeplitz_post.py on
'hip'): ``toeplitz_predict``, ``toeplitz_inverse_diagonal``, ``toeplitz_loo`` and the model layer on top.

The yardstick (``yardstick``): against a truth the device is at most 4 x the cpu backend's distance, with the floor 64 * 2^-53
relative to the largest magnitude of the quantity; on the ill-conditioned goldens also at most the distance of numpy's dense fp64
route on the same T.  Where an identity has an exact right-hand side, the truth is that right-hand side.  Every check takes the
backend and returns what it measured."""
import functools
import json
import os

import numpy as np
from scipy.linalg import cho_factor, cho_solve, solve_triangular, toeplitz

import gsum_amd as gm
import toeplitz_cases as tc
import toeplitz_grad_cases as gc
from toeplitz_cases import EPS, FLOOR, LD

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toeplitz_post.json")
H_STEP = 2.0 ** -6


def chunk_columns(n):
    """The device kernel's right-hand-side columns per workgroup (C) in the size class of n."""
    return 16 if n <= 512 else 12 if n <= 2048 else 5 if n <= 4096 else 3


def q_class(n):
    """2 C + 1 new points: a call crosses two chunk edges of k_schur and leaves a partial MFMA tile."""
    return 2 * chunk_columns(n) + 1


def golden_cols(n):
    return gc.cols_at(n)


def off_grid_points(n):
    """q_class(n) exactly representable positions in grid units: -3.25 and n + 0.5 outside, 5 + 2^-30, and half-integers inside."""
    m = q_class(n) - 3
    inside = [float((j * (n - 2)) // max(m - 1, 1)) + 0.5 for j in range(m)]
    assert len(set(inside)) == m and max(inside) < n - 1
    return [-3.25, n + 0.5, 5.0 + 2.0 ** -30] + inside


def lorentz_columns(n, s):
    """K[i, j] = 1 / (1 + ((i - s_j) h)^2), h = 2^-6, by +, -, *, / of Python floats in this order: bit-reproducible, no kernel build."""
    K = np.empty((n, len(s)))
    for j, sj in enumerate(s):
        for i in range(n):
            d = (float(i) - sj) * H_STEP
            K[i, j] = 1.0 / (1.0 + d * d)
    return K


def rel(a, b):
    """max |a - b| / max |b| in long double, as a float."""
    return gc.rel(a, b)


def numpy_pieces(t, K, Z):
    """numpy's dense fp64 route on the same T: (quad, cross, cov) from numpy.linalg.cholesky and two triangular solves."""
    L = np.linalg.cholesky(toeplitz(t))
    V, W = solve_triangular(L, K, lower=True), solve_triangular(L, Z, lower=True)
    return np.einsum("ij,ij->j", V, V), V.T @ W, V.T @ V


PIECES = ("quad", "cross", "cov")


def piece_distances(got, truth):
    return tuple(rel(g, w) for g, w in zip(got, truth))


def yardstick(cpu):
    """The bound on the device's distance from a truth, given the cpu backend's: 4 x that distance, and the floor 64 * 2^-53 where that
    is more.  toeplitz_cases._rule itself -- the floor times the cpu backend's factor over it, capped at 4 -- holds the device to the cpu
    backend's own distance once that lies between one and four floors and to four floors beyond; it was made for quantities the cpu
    backend has within the floor.  The identity's products with Z are not such: both backends run the substitution in fp64 and sit
    at cond(T) sqrt(n) roundings (100 floors at n = 8192), neither below the other throughout."""
    return max(4 * cpu, FLOOR)


def _under_golden_bounds(what, names, d, d_np, d_cpu):
    for k, name in enumerate(names):
        assert d[k] <= max(d_np[k], FLOOR), (what, name, d, d_np)
        assert d[k] <= 4 * max(d_cpu[k], FLOOR), (what, name, d, d_cpu)


# ---- (1): new points = training points ---------------------------------------------------------------------------------------------------

def identity_indices(n):
    """{0, 1, E - 1, E, n // 2, n - 2, n - 1} and further distinct indices, spread evenly and then in order, up to q_class(n) (n if that
    is fewer)."""
    E = tc.elements_per_thread(n)
    q = min(q_class(n), n)
    idx = []
    for i in [0, 1, E - 1, E, n // 2, n - 2, n - 1] + [(j * (n - 1)) // (q + 1) for j in range(1, q + 1)] + list(range(n)):
        if 0 <= i < n and i not in idx and len(idx) < q:
            idx.append(i)
    return np.array(idx)


def _identity_call(backend, t, Z):
    """The distances of the identity on one first column, with the bitwise checks: K = T[:, idx] gives quad = t_0, cross = Z[idx],
    cov = T[idx, idx]."""
    n = len(t)
    idx = identity_indices(n)
    K = t[np.abs(np.arange(n)[:, None] - idx[None, :])]
    r = gm.toeplitz_predict(t, K, Z, want_cov=True, backend=backend)
    q, c = len(idx), Z.shape[1]
    assert r.info == 0 and r.quad.shape == (q,) and r.cross.shape == (q, c) and r.cov.shape == (q, q) and r.G.shape == (c, c)
    assert np.array_equal(r.cov, r.cov.T)
    if backend != "cpu" or n < 4095:                                    # on the cpu backend G is _cpu_gram's by construction: seconds saved
        G, sld, info = gm.toeplitz_gram(t, Z, backend=backend)
        assert info == 0 and np.array_equal(r.G, G[0]) and r.sum_log_diag == sld
    return piece_distances((r.quad, r.cross, r.cov), (np.full(q, t[0]), Z[idx], K[idx])), (t, K, Z)


@functools.lru_cache(maxsize=None)
def identity_distances(backend, n):
    """The worst distances (quad, cross, cov) over the ARFIMA first columns of a size (both d below n = 4095, one from there on)."""
    ds, t, _, Z = gc._identity_inputs(n)
    d = [_identity_call(backend, ti, Z)[0] for ti in t]
    return tuple(max(x[k] for x in d) for k in range(3))


def check_identity(backend, n):
    """(1) on ARFIMA columns: under the yardstick against the cpu backend's own distances."""
    got, cpu = identity_distances(backend, n), identity_distances("cpu", n)
    print(f"toeplitz post identity {backend} n={n} q={min(q_class(n), n)}: " +
          ", ".join(f"{PIECES[k]} {got[k] / EPS:.2f} eps (cpu {cpu[k] / EPS:.2f})" for k in range(3)))
    for k in range(3):
        assert got[k] <= yardstick(cpu[k]), (n, PIECES[k], got, cpu)
    return dict(zip(PIECES, (g / EPS for g in got)))


def ill_case(name):
    return [c for c in tc.ill_cases() if c["name"] == name][0]


@functools.lru_cache(maxsize=None)
def _identity_golden(backend, name):
    case = ill_case(name)
    t = tc.hex_column(case)
    return _identity_call(backend, t, tc.rhs_columns(case["n"], golden_cols(case["n"])))


@functools.lru_cache(maxsize=None)
def _identity_golden_numpy(name):
    _, (t, K, Z) = _identity_golden("cpu", name)
    idx = identity_indices(len(t))
    return piece_distances(numpy_pieces(t, K, Z), (np.full(len(idx), t[0]), Z[idx], K[idx]))


def check_identity_golden(backend, name):
    """(1) on the ill-conditioned golden columns: within 4 x the cpu backend's distance, floor 64 * 2^-53.  The truth is the exact
    right-hand side, not a golden, so numpy's dense route is no bound here; its distance is printed beside the others (on the products
    with Z both routes are at cond(T) roundings of an fp64 substitution, and neither is the closer one throughout)."""
    d, d_cpu, d_np = _identity_golden(backend, name)[0], _identity_golden("cpu", name)[0], _identity_golden_numpy(name)
    print(f"toeplitz post identity golden {name} {backend}: " +
          ", ".join(f"{PIECES[k]} {d[k]:.3g} (numpy {d_np[k]:.3g}, cpu {d_cpu[k]:.3g})" for k in range(3)))
    for k in range(3):
        assert d[k] <= 4 * max(d_cpu[k], FLOOR), (name, PIECES[k], d, d_cpu)
    return d, d_np, d_cpu


# ---- (2): off-grid goldens against mpmath ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden():
    """toeplitz_post.json (names, sizes, the points s) with the answers of toeplitz_post.npz, "<name>/quad", "/cross", "/cov" and "/p"
    as float64, put into each case."""
    with open(GOLDEN) as f:
        g = json.load(f)
    with np.load(GOLDEN[:-5] + ".npz") as f:
        for case in g["cases"]:
            case.update({k: f[case["name"] + "/" + k] for k in ("quad", "cross", "cov", "p")})
    return g


def golden_case(name):
    return [c for c in golden()["cases"] if c["name"] == name][0]


def golden_names():
    return [c["name"] for c in golden()["cases"]]


@functools.lru_cache(maxsize=None)
def _offgrid_inputs(name):
    case = golden_case(name)
    n = case["n"]
    assert case["s"] == off_grid_points(n) and case["q"] == q_class(n) and case["cols"] == golden_cols(n)
    t, K, Z = tc.hex_column(ill_case(name)), lorentz_columns(n, case["s"]), tc.rhs_columns(n, case["cols"])
    truth = (np.array(case["quad"]), np.array(case["cross"]), np.array(case["cov"]))
    for a in (t, K, Z):
        a.setflags(write=False)
    return t, K, Z, truth, piece_distances(numpy_pieces(t, K, Z), truth)


@functools.lru_cache(maxsize=None)
def _offgrid_distances(backend, name):
    t, K, Z, truth, _ = _offgrid_inputs(name)
    r = gm.toeplitz_predict(t, K, Z, want_cov=True, backend=backend)
    assert r.info == 0 and np.array_equal(r.cov, r.cov.T)
    return piece_distances((r.quad, r.cross, r.cov), truth)


def check_offgrid(backend, name):
    """(2): quad, cross and cov of the off-grid columns against the mpmath truth, each at most numpy's dense route's distance on the
    same T (with the floor) and within 4 x the cpu backend's.  The cpu backend itself, which rounds L to fp64 in its substitution
    without the device's correction word, is one fp64 substitution beside another: it is held to 4 x numpy's distance, the
    yardstick's own factor between two implementations (on rbf_n2049 its quad and cov sit 17 % beyond numpy's)."""
    d, d_cpu, d_np = _offgrid_distances(backend, name), _offgrid_distances("cpu", name), _offgrid_inputs(name)[4]
    print(f"toeplitz post off-grid golden {name} {backend}: " +
          ", ".join(f"{PIECES[k]} {d[k]:.3g} (numpy {d_np[k]:.3g}, cpu {d_cpu[k]:.3g})" for k in range(3)))
    if backend == "cpu":
        for k in range(3):
            assert d[k] <= 4 * max(d_np[k], FLOOR), (name, PIECES[k], d, d_np)
    else:
        _under_golden_bounds(name, PIECES, d, d_np, d_cpu)
    return d, d_np, d_cpu


# ---- (3): p = diag(T^-1) ------------------------------------------------------------------------------------------------------------------

def prefix_diagonal(x):
    """p from x = T^-1 e_0 in long double: the running sums of (x_r - x_{n-r}) (x_r + x_{n-r}), x_n = 0, over x_0."""
    x = np.asarray(x, dtype=LD)
    xn = np.concatenate([[LD(0)], x[:0:-1]])
    return np.cumsum((x - xn) * (x + xn)) / x[0]


P_NAMES = ("p", "sum", "mirror")


@functools.lru_cache(maxsize=None)
def diagonal_distances(backend, n):
    """(3a), (3c), (3d) on the ARFIMA columns of a size: p against the prefix of the closed-form x, sum p against trace(T^-1) as
    ``toeplitz_grad(t, dt=[e_0])`` of the same backend gives it, and p_i against p_{n-1-i}; each relative to the largest magnitude."""
    ds, t, dt, Z = gc._identity_inputs(n)
    p, info = gm.toeplitz_inverse_diagonal(t, backend=backend)
    assert p.shape == t.shape and not info.any()
    trace = gm.toeplitz_grad(t, dt[:, 1:], Z[:, :1], backend=backend)[3]
    out = [0.0, 0.0, 0.0]
    for i, d in enumerate(ds):
        got = (rel(p[i], prefix_diagonal(gc.arfima_inverse_column(n, d))), float(abs(np.sum(p[i].astype(LD)) - trace[i, 0]) / abs(trace[i, 0])),
               rel(p[i], p[i][::-1]))
        out = [max(a, b) for a, b in zip(out, got)]
    p1, i1 = gm.toeplitz_inverse_diagonal(t[0], backend=backend)       # one first column: (n,) and a scalar, the same bits
    assert i1 == 0 and np.array_equal(p1, p[0])
    return tuple(out)


def check_diagonal(backend, n):
    got, cpu = diagonal_distances(backend, n), diagonal_distances("cpu", n)
    print(f"toeplitz post diagonal {backend} n={n}: " + ", ".join(f"{P_NAMES[k]} {got[k] / EPS:.2f} eps (cpu {cpu[k] / EPS:.2f})" for k in range(3)))
    for k in range(3):
        assert got[k] <= yardstick(cpu[k]), (n, P_NAMES[k], got, cpu)
    return dict(zip(P_NAMES, (g / EPS for g in got)))


@functools.lru_cache(maxsize=None)
def _diagonal_golden(backend, name):
    case = golden_case(name)
    t = tc.hex_column(ill_case(name))
    want = np.array(case["p"])
    if backend == "numpy":
        return rel(np.diag(cho_solve(cho_factor(toeplitz(t), lower=True), np.eye(len(t)))), want)
    p, info = gm.toeplitz_inverse_diagonal(t, backend=backend)
    assert info == 0
    return rel(p, want)


def check_diagonal_golden(backend, name):
    """(3b): p against mpmath on the ill-conditioned goldens: at most numpy's dense route's distance (with the floor) and within 4 x
    the cpu backend's."""
    d, d_np, d_cpu = (_diagonal_golden(b, name) for b in (backend, "numpy", "cpu"))
    print(f"toeplitz post diagonal golden {name} {backend}: p {d:.3g} (numpy {d_np:.3g}, cpu {d_cpu:.3g})")
    _under_golden_bounds(name, ("p",), (d,), (d_np,), (d_cpu,))
    return d, d_np, d_cpu


def check_diagonal_golden_extended(backend, name):
    """(3e), for the device alone, as toeplitz_grad_cases.check_golden_extended: x and the prefix are double-double there and long
    double on the cpu backend, so the device's p, rounded once, is held to 2^-20 of the cpu backend's distance, floor 64 * 2^-53.
    That floor does not see a lost low word of x: on these columns the prefix cancels by a factor of at most 101 (sum |terms| over
    |p_i|; measured in long double), so rounding x to fp64 moves p by 0.2 to 0.8 * 2^-53 of max |p|.  What does see it: 106 bits less
    those 7 leave the device's p 2^-90 from the truth before its one rounding, so on these fixed inputs it is the correctly rounded
    value, bit for bit the golden's (a truth within 2^-90 of a rounding boundary, one entry in 2^37, would show as one ulp here
    and be no fault of the kernel's)."""
    d, d_cpu = _diagonal_golden(backend, name), _diagonal_golden("cpu", name)
    bound = max(d_cpu * 2.0 ** -20, FLOOR)
    assert d <= bound, (name, d, d_cpu, bound)
    p, _ = gm.toeplitz_inverse_diagonal(tc.hex_column(ill_case(name)), backend=backend)
    off = np.flatnonzero(p != np.array(golden_case(name)["p"]))
    assert off.size == 0, (name, off.size, off[:5])
    return d


# ---- (4): properties ----------------------------------------------------------------------------------------------------------------------

def _pieces_equal(a, b, sel=None):
    """quad, cross and cov of two results, the second restricted to the new points ``sel``."""
    sel = slice(None) if sel is None else sel
    ok = np.array_equal(a.quad, b.quad[sel]) and np.array_equal(a.cross, b.cross[sel])
    if a.cov is not None and b.cov is not None:
        ok = ok and np.array_equal(a.cov, b.cov[sel][:, sel])
    return ok


def check_properties(backend, n):
    """(4): quad, cross and cov[a, b] do not depend bit for bit on the order of the new points, on which others are there, on the
    chunking, on whether cov is asked for or on the other residual columns; cov is bitwise symmetric; powers of two on K and Z and
    powers of four on t move the results by exact powers of two; the earlier entry points give the same bits before and after a
    ``toeplitz_predict`` call on the same handle, and their clocks are not charged by the new calls."""
    rng = np.random.RandomState(7)
    t1 = tc.kms_column(n, 0.5) + 0.25 * tc.kms_column(n, -0.5)
    q = q_class(n)
    K, Z = rng.randn(n, q), rng.randn(n, 3)
    full = gm.toeplitz_predict(t1, K, Z, want_cov=True, backend=backend)
    assert full.info == 0 and np.array_equal(full.cov, full.cov.T)
    assert _pieces_equal(gm.toeplitz_predict(t1, K, Z, want_cov=True, backend=backend), full)                  # two runs
    perm = rng.permutation(q)
    assert _pieces_equal(gm.toeplitz_predict(t1, K[:, perm], Z, want_cov=True, backend=backend), full, perm)   # permuted
    half = np.arange(0, q, 2)
    assert _pieces_equal(gm.toeplitz_predict(t1, K[:, half], Z, want_cov=True, backend=backend), full, half)   # half of them dropped
    chunked = gm.toeplitz_predict(t1, K, Z, chunk=5, backend=backend)
    assert chunked.cov is None and _pieces_equal(chunked, full) and np.array_equal(chunked.G, full.G)           # in calls of five
    assert chunked.sum_log_diag == full.sum_log_diag and chunked.info == 0
    assert _pieces_equal(gm.toeplitz_predict(t1, K, Z, backend=backend), full)                                 # without cov
    other = gm.toeplitz_predict(t1, K, np.concatenate([rng.randn(n, 4), Z[:, 1:2]], axis=1), want_cov=True, backend=backend)
    assert np.array_equal(other.quad, full.quad) and np.array_equal(other.cov, full.cov)                       # other residual columns
    assert np.array_equal(other.cross[:, 4], full.cross[:, 1])
    none = gm.toeplitz_predict(t1, K, None, want_cov=True, backend=backend)                                    # no residual column at all
    assert none.cross.shape == (q, 0) and none.G.shape == (0, 0) and np.array_equal(none.quad, full.quad) and np.array_equal(none.cov, full.cov)
    b = 7
    for a, j in tc.SCALINGS:
        sc = gm.toeplitz_predict(4.0 ** j * t1, 2.0 ** a * K, 2.0 ** b * Z, want_cov=True, backend=backend)
        assert sc.info == 0
        assert np.array_equal(sc.quad, 2.0 ** (2 * a - 2 * j) * full.quad) and np.array_equal(sc.cov, 2.0 ** (2 * a - 2 * j) * full.cov), (a, j)
        assert np.array_equal(sc.cross, 2.0 ** (a + b - 2 * j) * full.cross) and np.array_equal(sc.G, 2.0 ** (2 * b - 2 * j) * full.G), (a, j)
    if backend == "cpu" or n > 1000:
        return
    from gsum_amd import _toep_lib
    h = _toep_lib.default_handle(0)

    def earlier():
        out = []
        for ns, c, n_sets, m in tc.SHAPES:
            ts, Zs, _ = tc._kms_inputs(ns, c, n_sets, m)
            out += list(gm.toeplitz_gram(ts, Zs, n_sets, backend=backend))
            out += list(gm.toeplitz_grad(ts, ts[:, None, :], Zs, n_sets, backend=backend))
            out += list(gm.toeplitz_solve(ts[:2], Zs[:, :c], backend=backend))
        return out

    before = earlier()
    clocks = h.times(), h.grad_times()
    h.post_times(reset=True)
    gm.toeplitz_predict(t1, K, Z, want_cov=True, backend=backend)
    gm.toeplitz_loo(t1, Z, 0.25, backend=backend)
    assert (h.times(), h.grad_times()) == clocks                       # the new calls charge their own clock alone
    ms = h.post_times()
    assert tuple(ms) == _toep_lib.POST_PHASES and all(v > 0 for v in ms.values()), ms
    assert gc._same(earlier(), before)


# ---- (5): failures ------------------------------------------------------------------------------------------------------------------------

def check_late_failures(backend, n=513, d=0.25):
    """(5): a first column that fails at step p + 1 (toeplitz_cases.check_late_failures' construction) for p = 1, E and n - 1: info ==
    p + 1, every output NaN, no error; the inverse's diagonal likewise."""
    good = tc.arfima_column(n, d)
    En = tc.arfima_energies(n, d)
    rng = np.random.RandomState(5)
    K, Z = rng.randn(n, q_class(n)), tc.rhs_columns(n, 2)
    infos = []
    for p in (1, tc.elements_per_thread(n), n - 1):
        t = good.copy()
        t[p] += 1.5 * float(En[p - 1])
        r = gm.toeplitz_predict(t, K, Z, want_cov=True, backend=backend)
        assert r.info == p + 1, (p, r.info)
        assert all(np.isnan(a).all() for a in (r.quad, r.cross, r.cov, r.G)) and np.isnan(r.sum_log_diag)
        pd, info = gm.toeplitz_inverse_diagonal(t, backend=backend)
        assert info == p + 1 and np.isnan(pd).all()
        infos.append(int(r.info))
    r = gm.toeplitz_predict(good, K, Z, want_cov=True, backend=backend)
    assert r.info == 0 and all(np.isfinite(a).all() for a in (r.quad, r.cross, r.cov, r.G))
    return infos


def check_shape_refusals(backend):
    """(5): what the Python layer refuses, on either backend."""
    import pytest
    t = tc.kms_column(8, 0.5)
    with pytest.raises(ValueError, match="K must have shape"):
        gm.toeplitz_predict(t, np.ones((7, 2)), backend=backend)
    with pytest.raises(ValueError, match="K must have shape"):
        gm.toeplitz_predict(t, np.ones((8, 0)), backend=backend)
    with pytest.raises(ValueError, match="Z must have shape"):
        gm.toeplitz_predict(t, np.ones((8, 2)), np.ones((7, 1)), backend=backend)
    with pytest.raises(ValueError, match="at most 16"):
        gm.toeplitz_predict(t, np.ones((8, 2)), np.ones((8, 17)), backend=backend)
    with pytest.raises(ValueError, match="t must have shape"):
        gm.toeplitz_predict(np.stack([t, t]), np.ones((8, 2)), backend=backend)
    with pytest.raises(ValueError, match="limit of 5"):
        gm.toeplitz_predict(t, np.ones((8, 6)), want_cov=True, chunk=5, backend=backend)
    n = 8192                                                            # beyond the 256 MB of solved columns: 4096 - c new points at n = 8192
    assert gm.toeplitz.predict_chunk(n, 2) == 4094
    with pytest.raises(ValueError, match="limit of 4094"):
        gm.toeplitz_predict(tc.kms_column(n, 0.5), np.zeros((n, 4095)), np.zeros((n, 2)), want_cov=True, backend=backend)
    with pytest.raises(ValueError, match="y must be"):
        gm.toeplitz_loo(t, np.ones(7), backend=backend)
    with pytest.raises(ValueError, match="t must have shape"):
        gm.toeplitz_loo(np.stack([t, t]), np.ones(8), backend=backend)
    with pytest.raises(np.linalg.LinAlgError):
        gm.toeplitz_loo(np.ones(8), np.ones(8), backend=backend)


# ---- (6): leave-one-out -------------------------------------------------------------------------------------------------------------------

LOO_NAMES = ("mean", "var", "error", "logpdf")


def loo_column(n):
    """The first column of the well-conditioned model of toeplitz_grad_cases.MODEL_CLASSES (Matern-1/2 plus a white term) on
    linspace(0, 1, n), from scikit-learn on the host: the same bits for every backend."""
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    X = np.linspace(0, 1, n)[:, None]
    kern = Matern(0.2, nu=0.5) + WhiteKernel(1e-6)
    t = kern(X, X[:1])[:, 0]
    t[0] = kern.diag(X[:1])[0] + 1e-10
    return t


def loo_points(n):
    """Every point up to n = 65; from there on the two ends, the first thread boundary of the size class and the middle: a solve of
    the matrix without row and column i costs an O(n^3) factorisation per point."""
    if n <= 65:
        return np.arange(n)
    return np.unique([0, tc.elements_per_thread(n), n // 2, n - 1])


def _solve_without(t, cf, i, B):
    """(T without row and column i)^-1 B in long double, T well conditioned, B (n, k) with anything in row i; the answer has a zero
    there.  Refinement: the residual of the smaller system is formed explicitly in long double (a Toeplitz product with a zero at i)
    and the correction comes from LAPACK's fp64 factor ``cf`` of the whole T, bordered so that its entry i vanishes -- a preconditioner
    only: what the iteration converges to is fixed by the residual.  A step contracts the error by cond 2^-53; what is left is long
    double's own cond 2^-64, as after a Cholesky factorisation in long double: the last correction, which measures it, must lie below
    the yardstick's floor."""
    n = len(t)
    e = np.zeros(n)
    e[i] = 1.0
    w = cho_solve(cf, e)

    def approx(R):
        R = R.astype(float)
        R[i] = 0.0
        S = cho_solve(cf, R)
        S -= np.outer(w, S[i] / w[i])
        S[i] = 0.0
        return S.astype(LD)

    Bl = B.astype(LD)
    X = approx(Bl)
    for _ in range(3):
        dX = approx(Bl - gc.toeplitz_times_ld(t, X))
        X = X + dX
    assert np.max(np.abs(dX)) <= FLOOR * np.max(np.abs(X)), "the brute-force solve is not good to the floor of the yardstick"
    return X


@functools.lru_cache(maxsize=None)
def _loo_truth(n):
    """(t, y (n, 3), mean, points, the brute force at those points: leave row and column i out, solve) in long double."""
    t = loo_column(n)
    y = np.random.RandomState(1).randn(n, 3)
    mean = 0.1
    cf = cho_factor(toeplitz(t))
    pts = loo_points(n)
    mu, var = np.empty((len(pts), 3), dtype=LD), np.empty(len(pts), dtype=LD)
    for a, i in enumerate(pts):
        k = t[np.abs(np.arange(n) - i)].astype(LD)                     # column i of T, without its own entry
        k[i] = 0
        S = _solve_without(t, cf, i, np.concatenate([np.asarray(k, dtype=float)[:, None], y - mean], axis=1))
        var[a] = LD(t[0]) - k @ S[:, 0]
        mu[a] = LD(mean) + k @ S[:, 1:]
    resid = y[pts].astype(LD) - mu
    err = resid / np.sqrt(var)[:, None]
    logpdf = -0.5 * np.log(2 * LD(np.pi)) - 0.5 * np.log(var)[:, None] - 0.5 * err * err
    for a in (t, y):
        a.setflags(write=False)
    return t, y, mean, pts, (mu, var, err, logpdf)


def _loo_distances(res, pts, truth):
    return tuple(rel(np.asarray(getattr(res, name))[pts], w) for name, w in zip(LOO_NAMES, truth))


@functools.lru_cache(maxsize=None)
def loo_distances(backend, n):
    t, y, mean, pts, truth = _loo_truth(n)
    res = gm.toeplitz_loo(t, y, mean, backend=backend)
    assert res.mean.shape == (n, 3) and res.var.shape == (n,) and np.array_equal(res.var, 1.0 / res.precision_diag)
    one = gm.toeplitz_loo(t, y[:, 1], mean, backend=backend)            # one curve: (n,) throughout
    assert one.mean.shape == (n,) and np.array_equal(one.mean, res.mean[:, 1]) and np.array_equal(one.logpdf, res.logpdf[:, 1])
    return _loo_distances(res, pts, truth)


@functools.lru_cache(maxsize=None)
def loo_dense_distances(backend, n):
    """The distances of ``loo_from_factor`` on numpy's Cholesky factor of the same T from the same truth."""
    t, y, mean, pts, truth = _loo_truth(n)
    return _loo_distances(gm.loo_from_factor(np.linalg.cholesky(toeplitz(t)), y, mean, backend=backend), pts, truth)


def check_loo(backend, n):
    """(6): mean, var, error and logpdf against the brute force, under the yardstick and at most 4 x the dense route's distance."""
    d, d_cpu, d_dense = loo_distances(backend, n), loo_distances("cpu", n), loo_dense_distances(backend, n)
    print(f"toeplitz post loo {backend} n={n}: " + ", ".join(f"{LOO_NAMES[k]} {d[k] / EPS:.2f} eps (cpu {d_cpu[k] / EPS:.2f}, dense "
                                                            f"{d_dense[k] / EPS:.2f})" for k in range(4)))
    for k, name in enumerate(LOO_NAMES):
        assert d[k] <= yardstick(d_cpu[k]), (n, name, d, d_cpu)
        assert d[k] <= 4 * d_dense[k], (n, name, d, d_dense)
    return dict(zip(LOO_NAMES, (x / EPS for x in d)))


# ---- (7): the model layer -----------------------------------------------------------------------------------------------------------------

class DenseCounters:
    """Counts the calls of what builds or factorises an n x n matrix on a context while a fit runs (monkeypatch)."""

    NAMES = ("factorize", "kernel_matrix_dev", "potrf")

    def __init__(self, monkeypatch, ctx):
        self.calls = 0
        for name in self.NAMES:
            monkeypatch.setattr(ctx, name, self._wrap(getattr(ctx, name)), raising=True)

    def _wrap(self, fn):
        def counted(*a, **k):
            self.calls += 1
            return fn(*a, **k)
        return counted


def new_points(X):
    """Seven interior points, one outside each end, one training point."""
    return np.concatenate([np.linspace(0.05, 0.95, 7), [-0.1, 1.1], X[5]])[:, None]


POSTERIOR = ("center_", "disp_", "df_", "scale_", "cov_factor_")
PREDICT_CALLS = (dict(), dict(return_std=True), dict(return_cov=True), dict(pred_noise=True), dict(return_std=True, pred_noise=True),
                 dict(return_cov=True, pred_noise=True))


def _as_tuple(out):
    return out if isinstance(out, tuple) else (out,)


def _with_posterior_of(target, source):
    for name in POSTERIOR + ("cbar_sq_mean_",):
        setattr(target, name, getattr(source, name))
    return target


def check_model(backend, name, n, monkeypatch):
    """(7): fit(structure="toeplitz", dense_factor=False) builds and factorises nothing n x n and ends where the structured calibration
    ended; the three pieces of ``predict`` against a long-double truth on the exact Toeplitz matrix, at most 4 x max(the dense
    route's distance, the floor); ``predict(structure="toeplitz")`` of a densely fitted process with the same posterior gives the
    same bits; another conditioning grid; ``loo`` and ``sample_y`` follow the route.  Returns the pieces' distances."""
    import grad_truth as gt
    from gsum_amd.kernels import describe_kernel
    cls, kw = gc.model_class(name), dict(gc.MODEL_CLASSES)[name]
    X, y = gc.model_xy(n)
    dense = gc.model_process(cls, backend, **kw).fit(X, y, structure="toeplitz")
    assert dense._L_dev is not None and dense.structure_ is None                   # structure="toeplitz" alone still leaves a dense factor
    gp = gc.model_process(cls, backend, **kw)
    ctx = gp._context()
    with monkeypatch.context() as mpc:
        cnt = DenseCounters(mpc, ctx)
        gp.fit(X, y, structure="toeplitz", dense_factor=False)
        assert cnt.calls == 0, cnt.calls
    assert gp._L_dev is None and gp.corr_L_ is None and gp.structure_ == "toeplitz" and gp._fit_structure is None
    assert np.array_equal(gp.kernel_.theta, dense.kernel_.theta)
    for attr in POSTERIOR:
        a, b = np.asarray(getattr(gp, attr), dtype=float), np.asarray(getattr(dense, attr), dtype=float)
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 100 * gc.FACTR_EPS * np.max(np.abs(b)), (attr, a, b)
    optimum = gp.log_marginal_likelihood_batch([gp.kernel_.theta], structure="toeplitz", eval_gradient=True)[0][0]
    assert gp.log_marginal_likelihood_value_ == optimum

    # the pieces against a long-double truth on the exact Toeplitz matrix, with the library's own K
    Xs = new_points(X)
    desc = describe_kernel(gp.kernel_, 1)
    t = gm.toeplitz_column(gp.kernel_, X, gp.nugget, backend=backend)
    K = ctx.kernel_matrix(desc, X, Xs)
    resid = np.asarray(y, dtype=float) - gp.mean(X)[:, None]
    got = gm.toeplitz_predict(t, K, resid, want_cov=True, backend=backend)
    css, VtW, VtV = ctx.predict_terms(dense._L_dev, desc, X, Xs, rhs=resid, want_cov=True)
    Li = gt.inverse_lower_ld(gt.cholesky_ld(toeplitz(t)))
    B = Li @ np.concatenate([K, resid], axis=1).astype(LD)
    q = len(Xs)
    truth = (np.sum(B[:, :q] * B[:, :q], axis=0), B[:, :q].T @ B[:, q:], B[:, :q].T @ B[:, :q])
    d, d_dense = piece_distances((got.quad, got.cross, got.cov), truth), piece_distances((css, VtW, VtV), truth)
    print(f"toeplitz post model {backend} {name} n={n}: " + ", ".join(f"{PIECES[k]} {d[k] / EPS:.2f} eps (dense {d_dense[k] / EPS:.2f})" for k in range(3)))
    for k in range(3):
        assert d[k] <= 4 * max(d_dense[k], FLOOR), (name, PIECES[k], d, d_dense)

    # predict: every form, the dense route nearby, and bit for bit what a densely fitted process with this posterior gives on the route
    twin = _with_posterior_of(cls(kernel=gp.kernel_, backend=backend, optimizer=None, **kw).fit(X, y), gp)
    assert twin._L_dev is not None and twin.structure_ is None
    for call in PREDICT_CALLS:
        out = _as_tuple(gp.predict(Xs, **call))
        assert out[0].shape == (q, y.shape[1]) and all(np.isfinite(o).all() for o in out)
        if call.get("return_cov"):
            assert out[1].shape == (q, q) and np.array_equal(out[1], out[1].T)
        if call.get("return_std"):
            assert out[1].shape == (q,)
        for o, w in zip(out, _as_tuple(dense.predict(Xs, **call))):
            assert np.max(np.abs(o - w)) <= 1e-9 * np.max(np.abs(w)), call  # section 18: the two routes sit 7e-10 apart at the worst
        for o, w in zip(out, _as_tuple(twin.predict(Xs, structure="toeplitz", **call))):
            assert np.array_equal(o, w), call
        assert all(np.array_equal(o, w) for o, w in zip(out, _as_tuple(gp.predict(Xs, structure="toeplitz", **call))))
    # the pieces do not depend on the posterior at all: a densely fitted process takes the same quad and cov from the route
    mean_s, std_s = dense.predict(Xs, return_std=True, structure="toeplitz")
    mean_d, std_d = dense.predict(Xs, return_std=True)
    assert np.max(np.abs(std_s - std_d)) <= 1e-9 * np.max(np.abs(std_d)) and np.max(np.abs(mean_s - mean_d)) <= 1e-9 * np.max(np.abs(mean_d))

    # another uniform conditioning grid
    Xc = np.linspace(-0.2, 0.9, n // 2 + 1)[:, None]
    yc = np.random.RandomState(2).randn(len(Xc), y.shape[1])
    for call in (dict(return_std=True), dict(return_cov=True)):
        out, want = gp.predict(Xs, Xc=Xc, y=yc, **call), dense.predict(Xs, Xc=Xc, y=yc, **call)
        for o, w in zip(out, want):
            assert o.shape == w.shape and np.max(np.abs(o - w)) <= 1e-9 * np.max(np.abs(w)), call

    # refusals
    import pytest
    from sklearn.gaussian_process.kernels import RBF, DotProduct
    Xj = X.copy()
    Xj[7] += 1e-9
    with pytest.raises(ValueError, match="uniform grid"):
        gp.predict(Xs, Xc=Xj, y=y)
    with pytest.raises(ValueError, match="one-dimensional grid"):
        gp.predict(Xs, Xc=np.random.RandomState(0).rand(n, 2), y=y)
    with pytest.raises(ValueError, match="structure"):
        dense.predict(Xs, structure="circulant")
    dot = cls(kernel=RBF(0.2) * DotProduct(1.0), backend=backend, optimizer=None, **kw).fit(X, y)
    with pytest.raises(NotImplementedError, match="stationary"):
        dot.predict(Xs, structure="toeplitz")
    with pytest.raises(ValueError, match="dense_factor"):
        gc.model_process(cls, backend, **kw).fit(X, y, dense_factor=False)
    eig = gc.model_process(cls, backend, optimizer=None, decomposition="eig", **kw).fit(X, y, structure="toeplitz", dense_factor=False)
    with pytest.raises(ValueError, match="dense_factor"):
        eig.corr_L_
    if name == "gaussian":                                              # devices=, kfold and loo are the Gaussian class's alone
        with pytest.raises(ValueError, match="dense_factor"):
            gp.predict(Xs, devices=[0])
        with pytest.raises(ValueError, match="devices"):
            dense.predict(Xs, devices=[0], structure="toeplitz")
        with pytest.raises(ValueError, match="dense_factor"):
            gp.kfold(4)
        # loo follows the route: toeplitz_loo of cov_factor_ * t
        want = gm.toeplitz_loo(float(np.squeeze(gp.cov_factor_)) * t, y, gp.mean(X), backend=backend)
        for res in (gp.loo(), gp.loo(structure="toeplitz"), twin.loo(structure="toeplitz")):
            assert all(np.array_equal(a, b) for a, b in zip(res, want))
        for a, b in zip(gp.loo(), dense.loo()):
            assert np.max(np.abs(a - b)) <= 1e-9 * np.max(np.abs(b))
    else:
        with pytest.raises(NotImplementedError):
            gp.loo()

    # sample_y follows predict: mean + L z of the structured covariance, drawn as sample_y draws
    from sklearn.utils import check_random_state
    draws = gp.sample_y(Xs, n_samples=3, random_state=4, method="cholesky", jitter=1e-10)
    assert draws.shape == (q, y.shape[1], 3)
    mean, cov = gp.predict(Xs, return_cov=True)
    L = ctx.upload(cov + 1e-10 * np.eye(q))
    try:
        assert ctx.potrf(L) == 0
        Lz = ctx.tri_multiply(L, check_random_state(4).standard_normal((q, 3 * y.shape[1])))
    finally:
        L.free()
    for i in range(y.shape[1]):
        assert np.array_equal(draws[:, i, :], mean[:, i:i + 1] + Lz[:, 3 * i:3 * (i + 1)])
    # a later dense fit forgets the route
    assert gp.fit(X, y).structure_ is None and gp._L_dev is not None
    return dict(zip(PIECES, (x / EPS for x in d)))
