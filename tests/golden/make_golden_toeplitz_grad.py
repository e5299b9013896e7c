#!/usr/bin/env python3
"""Known answers of the Toeplitz gradient pieces -> tests/golden/toeplitz_grad.json (names, traces, H) and
tests/golden/toeplitz_grad.npz (the long vectors, as float64: "<name>/dt" (n,) and "<name>/alpha" (n, cols); 200 KB of bits that as
hex text were 600 KB).

For the eight ill-conditioned first columns of toeplitz.json (n = 64, 128) and toeplitz_classes.json (n = 513, 2049, 4097), with
dt = the derivative of the first column by the kernel's length scale (gsum_amd.toeplitz_gradient_columns; its bits are kept, as float64) and
Z = toeplitz_cases.rhs_columns(n, cols):  trace = tr(T^-1 dT),  alpha = T^-1 Z,  H = alpha^T dT alpha.

At n <= 128 the truth is the dense mpmath inverse.  Above that it is the O(n^2) route itself in mpmath: the Schur recursion's
reflection coefficients, Levinson's recursion for x = T^-1 e_0, the diagonal sums of Gohberg-Semencul, four triangular Toeplitz
products per column and a Toeplitz product per entry of H.  Before anything is written that route must reproduce the dense answers of
the five small cases to 1e-50 (relative to the largest magnitude of each quantity); the figures are printed.  Both run at WORK digits,
above the 60 the answers are held to, because the dense inverse of a matrix with a condition number of 1e12 loses that many of them.

    python tests/golden/make_golden_toeplitz_grad.py [--jobs N] [--cache DIR]
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

import mpmath as mp
import numpy as np
from sklearn.gaussian_process.kernels import RBF, Matern, WhiteKernel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import toeplitz_cases as tc  # noqa: E402

DIGITS = 60
WORK = 80
mp.mp.dps = WORK
COLS = {4097: 2}                                                       # two columns suffice at n = 4097; four elsewhere


def length_scale_column(expr, n):
    """(dt of the length scale (n,), its index in theta) for the kernel expression of a golden on linspace(0, 1, n)."""
    kernel = eval(expr, {"__builtins__": {}}, dict(RBF=RBF, Matern=Matern, WhiteKernel=WhiteKernel))
    names = [h.name for h in kernel.hyperparameters if not h.fixed]
    p = [i for i, name in enumerate(names) if name.endswith("length_scale")][0]
    return tc.gm.toeplitz_gradient_columns(kernel, np.linspace(0, 1, n)[:, None])[p], p


def mpf_list(v):
    return [mp.mpf(float(x)) for x in v]


def mp_inverse_column(t):
    """x = T^-1 e_0: the generator recursion for (rho, 1 / c), then Levinson's recursion in its normalised form."""
    n = len(t)
    rs = 1 / mp.sqrt(t[0])
    u = [v * rs for v in t]
    v = [mp.mpf(0)] + u[1:]
    A, B = [rs], [rs]
    for k in range(n - 1):
        rho = v[k + 1] / u[k]
        if not abs(rho) < 1:
            raise ValueError(f"the matrix does not factor at step {k + 2}")
        ic = 1 / mp.sqrt((1 - rho) * (1 + rho))
        us, vv = u[k:n - 1], v[k + 1:]
        u[k + 1:] = [(a - rho * b) * ic for a, b in zip(us, vv)]
        v[k + 1:] = [(b - rho * a) * ic for a, b in zip(us, vv)]
        Ae, Bs = A + [mp.mpf(0)], [mp.mpf(0)] + B
        A = [(a - rho * b) * ic for a, b in zip(Ae, Bs)]
        B = [(b - rho * a) * ic for a, b in zip(Ae, Bs)]
    return [a / u[n - 1] for a in A]


def mp_trace(x, dt):
    n = len(x)
    s = [mp.fdot(((n - d - 2 * m) * x[m], x[m + d]) for m in range(n - d)) / x[0] for d in range(n)]
    return dt[0] * s[0] + 2 * mp.fdot(zip(dt[1:], s[1:]))


def lower(a, w):
    """L(a) w."""
    return [mp.fdot(zip(a[i::-1], w[:i + 1])) for i in range(len(a))]


def lower_t(a, z):
    """L(a)^T z."""
    n = len(a)
    return [mp.fdot(zip(a[:n - j], z[j:])) for j in range(n)]


def mp_solve(x, z):
    xt = [mp.mpf(0)] + x[:0:-1]
    p, q = lower(x, lower_t(x, z)), lower(xt, lower_t(xt, z))
    return [(a - b) / x[0] for a, b in zip(p, q)]


def toeplitz_times(dt, a):
    n = len(a)
    return [mp.fdot(zip(dt[i::-1], a[:i + 1])) + mp.fdot(zip(dt[1:n - i], a[i + 1:])) for i in range(n)]


def structured(t, dt, Z):
    """(trace, alpha as c lists, H c x c) by the O(n^2) route."""
    x = mp_inverse_column(t)
    alpha = [mp_solve(x, mpf_list(Z[:, c])) for c in range(Z.shape[1])]
    Q = [toeplitz_times(dt, a) for a in alpha]
    H = [[mp.fdot(zip(a, q)) for q in Q] for a in alpha]
    return mp_trace(x, dt), alpha, H


def dense(t, dt, Z):
    n = len(t)
    T = mp.matrix(n, n)
    D = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            T[i, j], D[i, j] = t[abs(i - j)], dt[abs(i - j)]
    Ti = mp.inverse(T)
    trace = mp.fsum(Ti[i, j] * D[j, i] for i in range(n) for j in range(n))
    Zm = mp.matrix([[mp.mpf(float(v)) for v in row] for row in Z])
    Am = Ti * Zm
    Hm = Am.T * (D * Am)
    c = Z.shape[1]
    return trace, [[Am[i, a] for i in range(n)] for a in range(c)], [[Hm[a, b] for b in range(c)] for a in range(c)]


def worst(a, b):
    """max |a - b| / max |b| over two equally nested lists of mpf."""
    fa, fb = np.array(a, dtype=object).ravel(), np.array(b, dtype=object).ravel()
    return max(abs(p - q) for p, q in zip(fa, fb)) / max(abs(q) for q in fb)


def run(job):
    case, cache = job
    name, n = case["name"], case["n"]
    path = cache and os.path.join(cache, f"grad_{name}.json")
    if path and os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    mp.mp.dps = WORK
    t0 = time.time()
    cols = COLS.get(n, 4)
    t = mpf_list(tc.hex_column(case))
    dt64, p = length_scale_column(case["kernel"], n)
    dt, Z = mpf_list(dt64), tc.rhs_columns(n, cols)
    trace, alpha, H = structured(t, dt, Z)
    method = "recursion"
    if n <= 128:
        want = dense(t, dt, Z)
        d = [mp.nstr(worst([trace], [want[0]]), 3), mp.nstr(worst(alpha, want[1]), 3), mp.nstr(worst(H, want[2]), 3)]
        print(f"self-check {name}: the O(n^2) route against the dense inverse: trace {d[0]}, alpha {d[1]}, H {d[2]}", flush=True)
        assert all(mp.mpf(v) <= mp.mpf("1e-50") for v in d), (name, d)
        trace, alpha, H = want
        method = "dense"
    out = dict(name=name, n=n, cols=cols, kernel=case["kernel"], theta_index=p, method=method, dt_hex=[float(v).hex() for v in dt64],
               trace=float(trace), H=[[float(v) for v in row] for row in H], alpha=[[float(a[i]) for a in alpha] for i in range(n)])
    print(f"{name}: {time.time() - t0:.0f} s, trace {out['trace']!r}", flush=True)
    if path:
        with open(path, "w") as f:
            json.dump(out, f)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--cache", help="a directory that keeps each finished case")
    args = ap.parse_args()
    if args.cache:
        os.makedirs(args.cache, exist_ok=True)
    cases = sorted(tc.ill_cases(), key=lambda c: -c["n"])
    with multiprocessing.Pool(args.jobs) as pool:
        done = pool.map(run, [(c, args.cache) for c in cases], chunksize=1)
    done.sort(key=lambda r: (r["n"], r["name"]))
    assert all(r["method"] == "dense" for r in done if r["n"] <= 128) and sum(r["n"] <= 128 for r in done) == 5
    arrays = {}
    for r in done:
        arrays[r["name"] + "/dt"] = np.array([float.fromhex(v) for v in r.pop("dt_hex")])
        arrays[r["name"] + "/alpha"] = np.array(r.pop("alpha"))
    np.savez_compressed(os.path.join(HERE, "toeplitz_grad.npz"), **arrays)
    with open(os.path.join(HERE, "toeplitz_grad.json"), "w") as f:
        json.dump(dict(method=f"mpmath, answers held to {DIGITS} digits (computed at {WORK}) on the Toeplitz matrices of the fp64 columns t "
                              "(t_hex of toeplitz.json / toeplitz_classes.json) and dt (dt_hex), rounded to fp64 at the end; n <= 128: the "
                              "dense inverse; above: Schur coefficients, Levinson's recursion, Gohberg-Semencul, checked against the "
                              "dense answers at n <= 128 to 1e-50 (make_golden_toeplitz_grad.py)",
                       digits=DIGITS, inputs="Z = toeplitz_cases.rhs_columns(n, cols); dt = d t / d log(length_scale); dt and alpha are in "
                                             "toeplitz_grad.npz under <name>/dt and <name>/alpha", cases=done), f)


if __name__ == "__main__":
    main()
