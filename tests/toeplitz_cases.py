"""Shared cases of the Toeplitz likelihood path (test_toeplitz_cpu.py on backend='cpu', test_gpu_toeplitz.py on 'hip').

(a) Closed forms: the Kac-Murdock-Szego matrix t_k = rho^k has sum_j log L_jj = (n - 1) / 2 * log(1 - rho^2) and a tridiagonal inverse
    (diagonal [1, 1 + rho^2, ..., 1 + rho^2, 1] / (1 - rho^2), off-diagonal -rho / (1 - rho^2)), so any z^T T^-1 z' is an O(n) sum, taken
    here in numpy.longdouble.  Bound: the project's floor 64 * 2^-53, relative to max|G| and to max(1, |sum_log_diag|), times the factor
    by which the cpu backend's own distance exceeds the floor, capped at 4.
(b) Failures, (c) bitwise properties, (d) ill-conditioned goldens (tests/golden/toeplitz.json, mpmath truth).
Every check takes the backend and returns what it measured, so the GPU tests can record it."""
import functools
import json
import os

import numpy as np
from scipy.linalg import solve_triangular, toeplitz

import gsum_amd as gm

LD = np.longdouble
EPS = 2.0 ** -53
FLOOR = 64 * EPS
RHOS = (0.5, -0.25)
# 512 / 2048 / 4096: where the device kernel changes its elements per thread (1, 4, 8, 16) and the columns of a chunk (16, 12, 5, 3);
# 8192 is its limit (toeplitz_max_n); the powers of two around 64 .. 129 are the wave and Gram-lane edges
SIZES = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192)
# (n, c, n_sets, m): the column counts, set counts and first-column counts on a short list
SHAPES = ((129, 1, 1, 1), (65, 2, 3, 2), (64, 5, 80, 1), (63, 16, 3, 257), (1025, 16, 1, 1), (4097, 5, 3, 1), (513, 16, 3, 2))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toeplitz.json")


def rhs_columns(n, cols, seed=0):
    """n x cols right-hand sides: ones, alternating signs, a ramp, then seeded normals."""
    i = np.arange(n)
    basic = [np.ones(n), (-1.0) ** i, i / max(n - 1, 1)]
    rng = np.random.RandomState(seed)
    return np.stack([basic[c] if c < 3 else rng.randn(n) for c in range(cols)], axis=1)


def kms_column(n, rho):
    return float(rho) ** np.arange(n)


def kms_truth(n, rho, Z, n_sets=1):
    """(G (n_sets, c, c), sum_log_diag) of the KMS matrix in numpy.longdouble, rounded to fp64."""
    r = LD(rho)
    z = np.asarray(Z, dtype=LD).reshape(n, n_sets, -1)
    if n == 1:
        return np.einsum("ksa,ksb->sab", z, z).astype(float), 0.0
    d = np.full(n, 1 + r * r, dtype=LD)
    d[0] = d[-1] = 1
    G = np.einsum("ksa,ksb->sab", z * d[:, None, None], z) - r * (np.einsum("ksa,ksb->sab", z[:-1], z[1:]) + np.einsum("ksa,ksb->sab", z[1:], z[:-1]))
    return (G / (1 - r * r)).astype(float), float((n - 1) / LD(2) * np.log1p(-r * r))


def distances(G, sld, Gt, st):
    return float(np.max(np.abs(G - Gt)) / np.max(np.abs(Gt))), float(abs(sld - st) / max(1.0, abs(st)))


@functools.lru_cache(maxsize=None)
def _kms_inputs(n, c, n_sets, m):
    """(t (m, n) with rho alternating over RHOS, Z, [truth per first column]): made once, shared, never written to."""
    rhos = [RHOS[i % len(RHOS)] for i in range(m)]
    t = np.stack([kms_column(n, r) for r in rhos])
    Z = rhs_columns(n, c * n_sets)
    truth = {r: kms_truth(n, r, Z, n_sets) for r in set(rhos)}
    t.setflags(write=False)
    Z.setflags(write=False)
    return t, Z, [truth[r] for r in rhos]


@functools.lru_cache(maxsize=None)
def kms_distances(backend, n, c=4, n_sets=1, m=2):
    """The worst distances (G, sum_log_diag) of a backend from the closed form over the m first columns of a shape."""
    t, Z, truth = _kms_inputs(n, c, n_sets, m)
    G, sld, info = gm.toeplitz_gram(t, Z, n_sets, backend=backend)
    assert G.shape == (m, n_sets, c, c) and sld.shape == (m,) and info.shape == (m,)
    assert not info.any(), info
    assert np.array_equal(G, G.transpose(0, 1, 3, 2))
    d = [distances(G[i], sld[i], *truth[i]) for i in range(m)]
    return max(x[0] for x in d), max(x[1] for x in d)


def check_closed_form(backend, n, c=4, n_sets=1, m=2):
    """(a): the backend against the closed form, under the floor times the cpu backend's own factor (at most 4)."""
    got = kms_distances(backend, n, c, n_sets, m)
    cpu = kms_distances("cpu", n, c, n_sets, m)
    bounds = tuple(FLOOR * min(4.0, max(1.0, x / FLOOR)) for x in cpu)
    print(f"toeplitz closed form {backend} n={n} c={c} sets={n_sets} m={m}: G {got[0] / EPS:.2f} eps (cpu {cpu[0] / EPS:.2f}), "
          f"sum_log_diag {got[1] / EPS:.2f} eps (cpu {cpu[1] / EPS:.2f})")
    assert got[0] <= bounds[0] and got[1] <= bounds[1], (got, bounds)
    return got, cpu


def check_failures(backend):
    """(b): info of the first columns that do not factor, alone and beside a good one."""
    n = 8
    Z = rhs_columns(n, 2)
    nan5 = kms_column(n, 0.5)
    nan5[5] = np.nan
    bad = [(np.ones(n), 2), (np.r_[0.0, np.ones(n - 1)], 1), (np.r_[1.0, 2.0, np.zeros(n - 2)], 2), (np.r_[-1.0, np.zeros(n - 1)], 1), (nan5, None)]
    good = kms_column(n, 0.5)
    G0, s0, i0 = gm.toeplitz_gram(good, Z, backend=backend)
    assert i0 == 0
    for t, want in bad:
        G, sld, info = gm.toeplitz_gram(t, Z, backend=backend)
        assert (info == want) if want is not None else (1 <= info <= 6), (t, info)
        assert np.isnan(sld) and np.isnan(G).all()
    # all of them in one call around the good one: it is not disturbed
    G, sld, info = gm.toeplitz_gram(np.stack([b[0] for b in bad[:2]] + [good] + [b[0] for b in bad[2:]]), Z, backend=backend)
    assert info[2] == 0 and np.array_equal(G[2], G0) and sld[2] == s0
    assert list(info[[0, 1, 3, 4]]) == [2, 1, 2, 1] and 1 <= info[5] <= 6
    assert np.isnan(sld[[0, 1, 3, 4, 5]]).all()


def check_properties(backend, n=257):
    """(c): bitwise reproducibility, and independence of m, of the other sets, of their order and of the column chunking."""
    rng = np.random.RandomState(3)
    t1 = kms_column(n, 0.5) + 0.25 * kms_column(n, -0.5)
    c = 5
    Zs = rng.randn(80, n, c)                                           # 80 sets

    def flat(sets):
        return sets.transpose(1, 0, 2).reshape(n, -1)

    G1, s1, i1 = gm.toeplitz_gram(t1, flat(Zs[:1]), 1, backend=backend)
    assert i1 == 0
    G1b, s1b, _ = gm.toeplitz_gram(t1, flat(Zs[:1]), 1, backend=backend)
    assert np.array_equal(G1, G1b) and s1 == s1b                       # two runs
    many = np.stack([kms_column(n, 0.9 * np.cos(i)) for i in range(257)])
    many[100] = t1
    Gm, sm, im = gm.toeplitz_gram(many, flat(Zs[:1]), 1, backend=backend)
    assert not im.any() and np.array_equal(Gm[100], G1) and sm[100] == s1          # a theta alone and among 257
    G80, s80, _ = gm.toeplitz_gram(t1, flat(Zs), 80, backend=backend)
    assert np.array_equal(G80[0], G1[0]) and s80 == s1                              # a set alone and among 80
    Gr, _, _ = gm.toeplitz_gram(t1, flat(Zs[::-1]), 80, backend=backend)
    assert np.array_equal(Gr[::-1], G80)                                            # ... and with the sets reversed
    Z16 = rng.randn(n, 16)
    G16, s16, _ = gm.toeplitz_gram(t1, Z16, 1, backend=backend)
    for lo, hi in ((0, 5), (5, 10), (10, 16)):                                      # c = 16 at once and in calls of 5, 5 and 6
        Gp, sp, _ = gm.toeplitz_gram(t1, Z16[:, lo:hi], 1, backend=backend)
        assert np.array_equal(Gp[0], G16[0][lo:hi, lo:hi]) and sp == s16


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def ill_names():
    return [c["name"] for c in golden()["ill"]]


def hex_column(case):
    return np.array([float.fromhex(v) for v in case["t_hex"]])


@functools.lru_cache(maxsize=None)
def _ill_yardsticks(name):
    """(t, Z, truth G, truth sum_log_diag, distances of numpy's fp64 Cholesky of the same T, distances of the cpu backend)."""
    case = [c for c in golden()["ill"] if c["name"] == name][0]
    t, Z = hex_column(case), rhs_columns(case["n"], case["cols"])
    Gt, st = np.array(case["G"]), case["sum_log_diag"]
    L = np.linalg.cholesky(toeplitz(t))
    Y = solve_triangular(L, Z, lower=True)
    d_np = distances(Y.T @ Y, float(np.sum(np.log(np.diag(L)))), Gt, st)
    G, sld, info = gm.toeplitz_gram(t, Z, backend="cpu")
    assert info == 0
    return t, Z, Gt, st, d_np, distances(G[0], sld, Gt, st)


def check_ill(backend, name):
    """(d): the backend's distance from the mpmath truth is at most numpy's dense fp64 Cholesky's on the same T (with the floor), and
    within 4 x the cpu backend's."""
    t, Z, Gt, st, d_np, d_cpu = _ill_yardsticks(name)
    G, sld, info = gm.toeplitz_gram(t, Z, backend=backend)
    assert info == 0
    d = distances(G[0], sld, Gt, st)
    print(f"toeplitz golden {name} {backend}: G {d[0]:.3g} (numpy {d_np[0]:.3g}, cpu {d_cpu[0]:.3g}), sum_log_diag {d[1]:.3g} "
          f"(numpy {d_np[1]:.3g}, cpu {d_cpu[1]:.3g})")
    for k in range(2):
        assert d[k] <= max(d_np[k], FLOOR), (name, k, d, d_np)
        assert d[k] <= 4 * max(d_cpu[k], FLOOR), (name, k, d, d_cpu)
    return d, d_np, d_cpu


def notebook_process(g, cls, backend):
    """The fitted truncation process of tests/golden/notebook_grid.json and its thetas."""
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel
    X, y = np.array(g["X_train"]), np.array(g["y_train"])
    kern = RBF(0.2) + WhiteKernel(g["nugget"], noise_level_bounds="fixed")
    gp = cls(kernel=kern, ref=g["ref"], ratio=0.5, center=0, disp=0, df=1, scale=1, optimizer=None, backend=backend)
    gp.fit(X, y, orders=np.array(g["orders"]))
    return gp, [[t] for t in np.log(g["ls_vals"])]
