#!/usr/bin/env python3
"""Known answers of the Toeplitz path in its upper size classes -> tests/golden/toeplitz_classes.json.

make_golden_toeplitz.py factors the dense matrix in mpmath, O(n^3): out of reach at n = 4097.  Here the truth is the Schur recursion
itself with the forward substitution beside it, both in mpmath at 60 digits: O(n^2 c), a few minutes per first column at n = 4097
and a quarter of an hour at 8192 with mpmath's pure-Python backend.  Before anything is written the recursion must

  1. reproduce the five "ill" answers of toeplitz.json (G and sum_log_diag of the dense mpmath Cholesky) to one ulp of fp64, and
  2. reproduce the closed-form sum_log_diag of ARFIMA(0, d, 0), on the unrounded mpmath column, to 1e-30;

both are printed.  The file then holds

  "arfima": G = Z^T T^-1 Z of the fp64 column tests/toeplitz_cases.py: arfima_column(n, d) with Z = rhs_columns(n, 4), for d in DS at
            n = 513, 2049, 4097 and 8192 (the smallest n of the three upper size classes of the device kernel, and its limit), with
            the sum_log_diag of that fp64 column and of the closed form beside it (they agree far below an ulp);
  "ill":    one ill-conditioned first column per upper class (a smooth kernel on linspace(0, 1, n) plus a nugget; the bits of t in
            hex), its G, sum_log_diag and 2-norm condition number.  Each must satisfy, and main() asserts: numpy's dense Cholesky of
            toeplitz(t) succeeds and sits at least 1e-10 (relative to max|G|) from the truth, and the cpu backend returns info 0.

    python tests/golden/make_golden_toeplitz_classes.py [--no-8192] [--jobs N]
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

import mpmath as mp
import numpy as np
from scipy.linalg import solve_triangular, toeplitz
from sklearn.gaussian_process.kernels import RBF, Matern, WhiteKernel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import toeplitz_cases as tc  # noqa: E402

DIGITS = 60
mp.mp.dps = DIGITS
COLS = 4
ARFIMA_SIZES = (513, 2049, 4097, 8192)
# (name, kernel, n, nugget): chosen on the CPU for the three conditions above; the achieved condition numbers are in the file
ILL = [("matern52_n513", "Matern(0.2, nu=2.5)", 513, 1e-10), ("rbf_n2049", "RBF(0.2)", 2049, 1e-8),
       ("matern52_n4097", "Matern(0.2, nu=2.5)", 4097, 1e-10)]


def first_column(kernel, X, nugget):
    t = kernel(X, X[:1])[:, 0]
    t[0] = kernel.diag(X[:1])[0] + nugget
    return t


def mp_schur_gram(t, Z):
    """(G (c x c, mpf), sum_log_diag (mpf)) of the symmetric Toeplitz matrix of the first column t (floats or mpf) and the right-hand
    sides Z (n x c floats): the Schur recursion in the fixed frame (u_i = L_ik for i >= k at step k), y_k = z_k / L_kk and
    z_i -= L_ik y_k beside it, G = sum_k y_k y_k^T."""
    n, c = Z.shape
    tm = [v if isinstance(v, mp.mpf) else mp.mpf(float(v)) for v in t]
    rs = 1 / mp.sqrt(tm[0])
    u = [v * rs for v in tm]
    v = [mp.mpf(0)] + u[1:]
    R = [[mp.mpf(float(x)) for x in Z[:, a]] for a in range(c)]
    G = [[mp.mpf(0)] * c for _ in range(c)]
    sld = mp.mpf(0)
    for k in range(n):
        d = u[k]
        sld += mp.log(d)
        y = [R[a][k] / d for a in range(c)]
        for a in range(c):
            for b in range(a + 1):
                G[a][b] += y[a] * y[b]
        if k == n - 1:
            break
        col = u[k + 1:]
        for a in range(c):
            ya = y[a]
            R[a][k + 1:] = [r - x * ya for r, x in zip(R[a][k + 1:], col)]
        rho = v[k + 1] / u[k]
        if not abs(rho) < 1:
            raise ValueError(f"the matrix does not factor at step {k + 2}")
        ic = 1 / mp.sqrt((1 - rho) * (1 + rho))
        us, vv = u[k:n - 1], v[k + 1:]
        u[k + 1:] = [(a - rho * b) * ic for a, b in zip(us, vv)]
        v[k + 1:] = [(b - rho * a) * ic for a, b in zip(us, vv)]
    for a in range(c):
        for b in range(a):
            G[b][a] = G[a][b]
    return G, sld


def rounded(G, sld):
    return [[float(x) for x in row] for row in G], float(sld)


def ulps(a, b):
    """The largest distance in ulps of fp64 over the entries.  An entry that is zero by symmetry (ones^T T^-1 alternating at even n: T^-1
    is centrosymmetric) holds the noise of 60 digits in either computation, 1e-55; such entries, below 1e-40 of the largest, must be
    that small in both and are left out of the ulp count."""
    a, b = np.atleast_1d(np.asarray(a, dtype=float)), np.atleast_1d(np.asarray(b, dtype=float))
    big = np.maximum(np.abs(a), np.abs(b))
    noise = big < 1e-40 * np.max(big)
    return float(np.max(np.where(noise, 0.0, np.abs(a - b) / np.spacing(big))))


def check_old_goldens():
    """Self-check 1: the recursion against the dense mpmath Cholesky of toeplitz.json, in ulps of fp64."""
    worst = 0.0
    for case in tc.golden()["ill"]:
        G, sld = rounded(*mp_schur_gram(tc.hex_column(case), tc.rhs_columns(case["n"], case["cols"])))
        du = ulps(G, case["G"]), ulps(sld, case["sum_log_diag"])
        print(f"self-check 1: {case['name']}: G {du[0]:.0f} ulp, sum_log_diag {du[1]:.0f} ulp of the dense mpmath answers", flush=True)
        worst = max(worst, *du)
    assert worst <= 1, worst
    print("self-check 1 passed: the five committed answers are reproduced to one ulp", flush=True)


def mp_arfima(n, d):
    """(the unrounded column, the closed-form sum_log_diag) of ARFIMA(0, d, 0) for the fp64 number d, in mpmath."""
    dm = mp.mpf(float(d))
    t = [mp.mpf(1)]
    for k in range(1, n):
        t.append(t[-1] * (k - 1 + dm) / (k - dm))
    return t, mp.fsum((n - k) * mp.log1p(-(dm / (k - dm)) ** 2) for k in range(1, n)) / 2


def check_closed_form():
    """Self-check 2: the recursion on the unrounded ARFIMA column against sum_j log L_jj = 1/2 sum_k (n - k) log1p(-gamma_k^2)."""
    worst = mp.mpf(0)
    for d in tc.DS + (0.25,):
        for n in (5, 200):
            t, want = mp_arfima(n, d)
            _, sld = mp_schur_gram(t, np.ones((n, 1)))
            err = abs(sld - want)
            print(f"self-check 2: ARFIMA d={d} n={n}: |sum_log_diag - closed form| = {mp.nstr(err, 3)}", flush=True)
            worst = max(worst, err)
    assert worst <= mp.mpf("1e-30"), worst
    print("self-check 2 passed: the closed form is reproduced to 1e-30", flush=True)


def run_arfima(job):
    n, d = job
    t0 = time.time()
    G, sld = rounded(*mp_schur_gram(tc.arfima_column(n, d), tc.rhs_columns(n, COLS)))
    closed = float(mp_arfima(n, d)[1])
    print(f"arfima n={n} d={d}: {time.time() - t0:.0f} s, sum_log_diag {sld!r} (closed form {closed!r})", flush=True)
    return dict(n=n, d=d, cols=COLS, G=G, sum_log_diag=sld, sum_log_diag_closed_form=closed)


def run_ill(job):
    name, expr, n, nugget = job
    t0 = time.time()
    env = dict(RBF=RBF, Matern=Matern, WhiteKernel=WhiteKernel)
    t = first_column(eval(expr, {"__builtins__": {}}, env), np.linspace(0, 1, n)[:, None], nugget)
    Z = tc.rhs_columns(n, COLS)
    G, sld = rounded(*mp_schur_gram(t, Z))
    T = toeplitz(t)
    w = np.linalg.eigvalsh(T)
    L = np.linalg.cholesky(T)                                          # condition: must succeed
    Y = solve_triangular(L, Z, lower=True)
    d_np = tc.distances(Y.T @ Y, float(np.sum(np.log(np.diag(L)))), np.array(G), sld)
    Gc, sc, info = tc.gm.toeplitz_gram(t, Z, backend="cpu")
    d_cpu = tc.distances(Gc[0], sc, np.array(G), sld)
    print(f"ill {name}: {time.time() - t0:.0f} s, cond {w[-1] / w[0]:.3g}, numpy's distance G {d_np[0]:.3g} sum_log_diag {d_np[1]:.3g}, "
          f"cpu backend's G {d_cpu[0]:.3g} sum_log_diag {d_cpu[1]:.3g}, info {info}", flush=True)
    assert info == 0 and d_np[0] >= 1e-10, (name, info, d_np)
    return dict(name=name, kernel=expr, n=n, grid="linspace(0, 1, n)", nugget=nugget, cols=COLS, cond=float(w[-1] / w[0]),
                t_hex=[float(v).hex() for v in t], G=G, sum_log_diag=sld)


def run(job):
    """One item; with --cache DIR its result is kept there, so a run that was cut short does not start again from nothing."""
    kind, arg, cache = job
    path = cache and os.path.join(cache, f"{kind}_{arg[0]}_{arg[-1]}.json")
    if path and os.path.exists(path):
        with open(path) as f:
            return kind, json.load(f)
    out = (run_arfima if kind == "arfima" else run_ill)(arg)
    if path:
        with open(path, "w") as f:
            json.dump(out, f)
    return kind, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-8192", action="store_true", help="leave the n = 8192 ARFIMA golden out (the longest item)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--cache", help="a directory that keeps each finished item")
    args = ap.parse_args()
    check_closed_form()
    check_old_goldens()
    if args.cache:
        os.makedirs(args.cache, exist_ok=True)
    sizes = [n for n in ARFIMA_SIZES if not (args.no_8192 and n == 8192)]
    jobs = [("arfima", (n, d), args.cache) for n in sorted(sizes, reverse=True) for d in tc.DS]
    jobs += [("ill", j, args.cache) for j in sorted(ILL, key=lambda j: -j[2])]
    with multiprocessing.Pool(args.jobs) as pool:
        done = pool.map(run, jobs, chunksize=1)
    arfima = sorted((r for kind, r in done if kind == "arfima"), key=lambda r: (r["n"], -r["d"]))
    ill = sorted((r for kind, r in done if kind == "ill"), key=lambda r: r["n"])
    with open(os.path.join(HERE, "toeplitz_classes.json"), "w") as f:
        json.dump(dict(method=f"the Schur recursion with the forward substitution beside it in mpmath at {DIGITS} digits on the Toeplitz "
                              "matrix of the fp64 first column, rounded to fp64 at the end (make_golden_toeplitz_classes.py); checked "
                              "against the dense mpmath Cholesky answers of toeplitz.json (one ulp) and the ARFIMA closed form (1e-30)",
                       digits=DIGITS,
                       inputs="arfima: t = toeplitz_cases.arfima_column(n, d), Z = toeplitz_cases.rhs_columns(n, 4); ill: t_hex (the "
                              "kernel on linspace(0, 1, n), nugget on t[0]), Z = toeplitz_cases.rhs_columns(n, 4); cond is the 2-norm "
                              "condition number of toeplitz(t) from numpy's eigvalsh",
                       arfima=arfima, ill=ill), f)


if __name__ == "__main__":
    main()
