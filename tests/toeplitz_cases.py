"""Shared cases of the Toeplitz likelihood path (test_toeplitz_cpu.py on backend='cpu', test_gpu_toeplitz.py on 'hip').

(a) Closed forms: the Kac-Murdock-Szego matrix t_k = rho^k has sum_j log L_jj = (n - 1) / 2 * log(1 - rho^2) and a tridiagonal inverse
    (diagonal [1, 1 + rho^2, ..., 1 + rho^2, 1] / (1 - rho^2), off-diagonal -rho / (1 - rho^2)), so any z^T T^-1 z' is an O(n) sum, taken
    here in numpy.longdouble.  Bound: the project's floor 64 * 2^-53, relative to max|G| and to max(1, |sum_log_diag|), times the factor
    by which the cpu backend's own distance exceeds the floor, capped at 4.
(b) Failures, (c) bitwise properties, (d) ill-conditioned goldens (tests/golden/toeplitz.json at n = 64 and 128, toeplitz_classes.json at
    the smallest n of the device kernel's three upper size classes; mpmath truth).
(e) A closed-form family whose every step rotates, ARFIMA(0, d, 0); (f) failures at late steps, at thread boundaries and in the last
    step; (g) the host loop over chunks of first columns; (h) scaling of t and Z, and right-hand sides beyond fp32's range.
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


def ill_cases():
    """The ill-conditioned goldens: those of toeplitz.json (n = 64, 128) and those of toeplitz_classes.json (n = 513, 2049, 4097)."""
    return golden()["ill"] + classes_golden()["ill"]


def ill_names():
    return [c["name"] for c in ill_cases()]


def hex_column(case):
    return np.array([float.fromhex(v) for v in case["t_hex"]])


@functools.lru_cache(maxsize=None)
def _ill_yardsticks(name):
    """(t, Z, truth G, truth sum_log_diag, distances of numpy's fp64 Cholesky of the same T, distances of the cpu backend)."""
    case = [c for c in ill_cases() if c["name"] == name][0]
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


# ---- (e) ARFIMA(0, d, 0): a closed-form family whose every step rotates -------------------------------------------------------------
# t_0 = 1, t_k = t_{k-1} (k - 1 + d) / (k - d) has the reflection coefficients gamma_k = d / (k - d): none vanishes, they decay like 1 / k.
# The KMS family above is an AR(1) process: gamma_1 = rho and every later coefficient is exactly 0, so after the first step of the
# recursion v is identically zero and the rotation a pure shift.  This family is the accuracy test of the rotation itself.
DS = (0.4, -0.3)
CLASSES_GOLDEN = os.path.join(os.path.dirname(GOLDEN), "toeplitz_classes.json")


def arfima_column(n, d):
    """The autocovariances of ARFIMA(0, d, 0) scaled to t_0 = 1, by +, -, *, / of Python floats in this order: bit-reproducible."""
    t = [1.0]
    for k in range(1, n):
        t.append(t[-1] * (k - 1 + d) / (k - d))
    return np.array(t)


def arfima_energies(n, d):
    """E_p = t_0 prod_{k <= p} (1 - gamma_k^2), p = 0 .. n - 1 (numpy.longdouble): the squared pivots of the recursion."""
    k = np.arange(1, n, dtype=LD)
    g = LD(d) / (k - LD(d))
    return np.concatenate([[LD(1)], np.cumprod((1 - g) * (1 + g))])


def arfima_sum_log_diag(n, d):
    """sum_j log L_jj = 1/2 sum_{k=1}^{n-1} (n - k) log1p(-gamma_k^2) in numpy.longdouble, rounded to fp64."""
    k = np.arange(1, n, dtype=LD)
    g = LD(d) / (k - LD(d))
    return float(np.sum((n - k) * np.log1p(-g * g)) / 2)


@functools.lru_cache(maxsize=None)
def classes_golden():
    with open(CLASSES_GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _arfima_inputs(n):
    """(t (2, n) with d over DS, Z (n, 4), closed-form sum_log_diag per first column, golden G (2, 4, 4) or None)."""
    t = np.stack([arfima_column(n, d) for d in DS])
    Z = rhs_columns(n, 4)
    gold = {c["d"]: np.array(c["G"]) for c in classes_golden()["arfima"] if c["n"] == n}
    t.setflags(write=False)
    Z.setflags(write=False)
    return t, Z, [arfima_sum_log_diag(n, d) for d in DS], (np.stack([gold[d] for d in DS]) if gold else None)


@functools.lru_cache(maxsize=None)
def _arfima_results(backend, n):
    t, Z, _, _ = _arfima_inputs(n)
    G, sld, info = gm.toeplitz_gram(t, Z, 1, backend=backend)
    assert G.shape == (2, 1, 4, 4) and not info.any(), info
    assert np.array_equal(G, G.transpose(0, 1, 3, 2))
    G.setflags(write=False)
    return G[:, 0], sld


def _rule(cpu):
    """The bound of (a): the floor times the factor by which the cpu backend exceeds it, at most 4."""
    return FLOOR * min(4.0, max(1.0, cpu / FLOOR))


def arfima_golden_sizes():
    return sorted({c["n"] for c in classes_golden()["arfima"]})


def check_arfima(backend, n):
    """(e): sum_log_diag against the closed form at every size, under the rule of (a); the cpu backend itself within the floor (that
    is: rounding t to fp64 does not move the answer).  G against the mpmath golden of tests/golden/toeplitz_classes.json where there is
    one (n = 513, 2049, 4097, 8192: the smallest n of the three upper size classes and the limit), under the same rule.  At the other
    sizes G has no truth: the backend is held to the cpu backend's G within the sum of the two bounds, 2 * 4 * 64 * 2^-53 of max|G|.
    That is a comparison of two implementations of one recursion, not a truth."""
    t, Z, st, Gt = _arfima_inputs(n)
    G, sld = _arfima_results(backend, n)
    Gc, sc = _arfima_results("cpu", n)
    d_s = max(abs(sld[i] - st[i]) / max(1.0, abs(st[i])) for i in range(2))
    c_s = max(abs(sc[i] - st[i]) / max(1.0, abs(st[i])) for i in range(2))
    out = dict(sld_eps=d_s / EPS, cpu_sld_eps=c_s / EPS)
    if Gt is not None:
        d_g = max(float(np.max(np.abs(G[i] - Gt[i])) / np.max(np.abs(Gt[i]))) for i in range(2))
        c_g = max(float(np.max(np.abs(Gc[i] - Gt[i])) / np.max(np.abs(Gt[i]))) for i in range(2))
        out.update(G_eps=d_g / EPS, cpu_G_eps=c_g / EPS)
    else:
        d_g = max(float(np.max(np.abs(G[i] - Gc[i])) / np.max(np.abs(Gc[i]))) for i in range(2))
        out.update(G_vs_cpu_eps=d_g / EPS)
    print(f"toeplitz arfima {backend} n={n}: " + ", ".join(f"{k} {v:.2f}" for k, v in out.items()))
    assert c_s <= FLOOR, (n, c_s)
    assert d_s <= _rule(c_s), (n, d_s, c_s)
    if Gt is not None:
        assert d_g <= _rule(c_g), (n, d_g, c_g)
    else:
        assert d_g <= 2 * 4 * FLOOR, (n, d_g)
    return out


# ---- (f) failures at late steps, next to thread boundaries and in the last step ------------------------------------------------------
LATE_SIZES = (513, 2049, 4097)


def elements_per_thread(n):
    """The device kernel's generator elements per thread (E) in the size class of n."""
    return 1 if n <= 512 else 4 if n <= 2048 else 8 if n <= 4096 else 16


def late_positions(n):
    E = elements_per_thread(n)
    J = (n // E) // 2
    return [1, 2, E - 1, E, E + 1, J * E - 1, J * E, J * E + 1, n - 2, n - 1], J * E + 1


def check_late_failures(backend, n, d=0.25):
    """(f): gamma_p is affine in t_p with the slope 1 / E_{p-1}, so adding 1.5 E_{p-1} to t_p of an ARFIMA column makes |gamma_p| about
    1.5 and leaves the earlier coefficients alone: info == p + 1.  The positions are the first steps, those around the first thread
    boundary (E) and around one in the middle (J E), and the last two; a NaN at t[J E + 1] fails at J E + 2.  All bad columns go in one
    call around the unedited one, which must come out bit for bit as from a call of its own."""
    good = arfima_column(n, d)
    En = arfima_energies(n, d)
    ps, p_nan = late_positions(n)
    bad = []
    for p in ps:
        t = good.copy()
        t[p] += 1.5 * float(En[p - 1])
        bad.append(t)
    t = good.copy()
    t[p_nan] = np.nan
    bad.append(t)
    want = [p + 1 for p in ps] + [p_nan + 1]
    half = len(bad) // 2
    Z = rhs_columns(n, 2)
    G0, s0, i0 = gm.toeplitz_gram(good, Z, backend=backend)
    assert i0 == 0
    G, sld, info = gm.toeplitz_gram(np.stack(bad[:half] + [good] + bad[half:]), Z, backend=backend)
    assert list(info) == want[:half] + [0] + want[half:], (n, list(info))
    rest = np.arange(len(info)) != half
    assert np.isnan(sld[rest]).all() and np.isnan(G[rest]).all()
    assert np.array_equal(G[half], G0) and sld[half] == s0
    return [int(x) for x in info]


# ---- (g) the host loop over chunks of first columns -----------------------------------------------------------------------------------
Y_BUDGET = 256 << 20                     # bytes of solved columns in flight (gsum_toep.hip: kYBudget)
CHUNKED = dict(n=513, c=16, n_sets=2045, m=3)


def first_columns_per_launch(n, ncols, m, budget=Y_BUDGET):
    """The library's arithmetic: how many first columns one launch of the recursion takes."""
    return max(1, min(m, 65535, budget // (n * ncols * 8)))


def check_chunk_loop(backend):
    """(g): a call whose solved columns exceed the library's budget, so that its three first columns go through one per launch
    (offsets into t, sum_log_diag, info and G; Y reused).  The middle one fails at step 3.  For each good one, G of the first, middle
    and last set and sum_log_diag are bitwise those of a call with that column and those three sets alone.  Device only (135 MB of Z)."""
    n, c, n_sets, m = (CHUNKED[k] for k in ("n", "c", "n_sets", "m"))
    assert first_columns_per_launch(n, n_sets * c, m) == 1
    goods = [arfima_column(n, d) for d in DS]
    bad = goods[0].copy()
    p = 2
    bad[p] += 1.5 * float(arfima_energies(n, DS[0])[p - 1])
    Z = np.asfortranarray(np.random.RandomState(11).standard_normal((n_sets * c, n)).T)
    G, sld, info = gm.toeplitz_gram(np.stack([goods[0], bad, goods[1]]), Z, n_sets, backend=backend)
    assert list(info) == [0, p + 1, 0], info
    assert np.isnan(sld[1]) and np.isnan(G[1]).all()
    pick = [0, n_sets // 2, n_sets - 1]
    Z3 = np.concatenate([Z[:, s * c:(s + 1) * c] for s in pick], axis=1)
    for i, t in ((0, goods[0]), (2, goods[1])):
        Gs, ss, is_ = gm.toeplitz_gram(t, Z3, 3, backend=backend)
        assert is_ == 0 and np.array_equal(G[i][pick], Gs) and sld[i] == ss, i
        assert np.isfinite(G[i]).all()
    return [int(x) for x in info]


# ---- (h) scaling, and the range of the fp32 correction word --------------------------------------------------------------------------
SCALINGS = ((40, 0), (-40, 0), (0, 20), (0, -20), (30, -15))
FAR = (140, -140)


def check_scaling(backend, name="matern52_n64"):
    """(h): G(2^a Z, 4^j t) == 2^(2a - 2j) G(Z, t) bit for bit (a power of 4 keeps 1 / sqrt(t_0) exactly scaled) and sum_log_diag moves by
    n j ln 2 within the floor.  On the golden where the fp32 correction word for the low words of L matters."""
    t, Z, Gt, st, d_np, d_cpu = _ill_yardsticks(name)
    n = t.size
    G0, s0, i0 = gm.toeplitz_gram(t, Z, backend=backend)
    assert i0 == 0
    worst = 0.0
    for a, j in SCALINGS:
        G, s, info = gm.toeplitz_gram(4.0 ** j * t, 2.0 ** a * Z, backend=backend)
        assert info == 0
        assert np.array_equal(G, 2.0 ** (2 * a - 2 * j) * G0), (a, j)
        want = s0 + n * j * np.log(2.0)
        worst = max(worst, abs(s - want) / max(1.0, abs(want)))
        assert abs(s - want) <= FLOOR * max(1.0, abs(want)), (a, j, s, want)
    return worst


def check_far_scaling(backend, a, name="matern52_n64"):
    """(h): right-hand sides scaled by 2^a with |a| = 140, beyond what an fp32 word holds: finite, info 0, and after scaling back inside
    the two bounds of (d)."""
    t, Z, Gt, st, d_np, d_cpu = _ill_yardsticks(name)
    G, sld, info = gm.toeplitz_gram(t, 2.0 ** a * Z, backend=backend)
    assert info == 0 and np.isfinite(G).all() and np.isfinite(sld), (a, info)
    d = distances(G[0] * 2.0 ** (-2 * a), sld, Gt, st)
    print(f"toeplitz far scaling {backend} a={a}: G {d[0]:.3g} (numpy {d_np[0]:.3g}, cpu {d_cpu[0]:.3g}), sum_log_diag {d[1]:.3g}")
    for k in range(2):
        assert d[k] <= max(d_np[k], FLOOR), (a, k, d, d_np)
        assert d[k] <= 4 * max(d_cpu[k], FLOOR), (a, k, d, d_cpu)
    return d


def notebook_process(g, cls, backend):
    """The fitted truncation process of tests/golden/notebook_grid.json and its thetas."""
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel
    X, y = np.array(g["X_train"]), np.array(g["y_train"])
    kern = RBF(0.2) + WhiteKernel(g["nugget"], noise_level_bounds="fixed")
    gp = cls(kernel=kern, ref=g["ref"], ratio=0.5, center=0, disp=0, df=1, scale=1, optimizer=None, backend=backend)
    gp.fit(X, y, orders=np.array(g["orders"]))
    return gp, [[t] for t in np.log(g["ls_vals"])]
