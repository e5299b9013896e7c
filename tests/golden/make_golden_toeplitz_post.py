#!/usr/bin/env python3
"""Known answers of the posterior pieces of the Toeplitz path -> tests/golden/toeplitz_post.json (names, sizes,
the points s) and tests/golden/toeplitz_post.npz (the answers as float64: "<name>/quad", "/cross", "/cov", "/p").

For the eight ill-conditioned first columns of toeplitz.json (n = 64, 128) and toeplitz_classes.json (n = 513, 2049, 4097), with the
off-grid columns K = toeplitz_post_cases.lorentz_columns(n, s) at the points s = toeplitz_post_cases.off_grid_points(n) (both kept out
of the file: the test rebuilds them bit for bit; the file holds s) and Z = toeplitz_cases.rhs_columns(n, cols):

    quad = diag(K^T T^-1 K),  cross = K^T T^-1 Z,  cov = K^T T^-1 K,  p = diag(T^-1).

At n <= 128 the truth is the dense mpmath inverse.  Above that it is the O(n^2) route in mpmath: the Schur recursion with the forward
substitution of [K | Z] beside it (make_golden_toeplitz_classes.mp_schur_gram) and, for p, Levinson's recursion for x = T^-1 e_0
(make_golden_toeplitz_grad.mp_inverse_column) with the Gohberg-Semencul prefix p_i = (1 / x_0) sum_{r <= i} (x_r^2 - x_{n-r}^2).  Before
anything is written that route must reproduce the dense answers of the five small cases to 1e-50 (relative to the largest magnitude of
each quantity); the figures are printed.  Everything runs at WORK digits, above the 60 the answers are held to.

    python tests/golden/make_golden_toeplitz_post.py [--jobs N] [--cache DIR]
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import toeplitz_cases as tc  # noqa: E402
import toeplitz_post_cases as pc  # noqa: E402
from make_golden_toeplitz_classes import mp_schur_gram  # noqa: E402
from make_golden_toeplitz_grad import mp_inverse_column, mpf_list, worst  # noqa: E402

DIGITS = 60
WORK = 80


def structured(t, KZ):
    """(the Gram matrix of [K | Z] under T^-1, p) by the O(n^2) routes."""
    G, _ = mp_schur_gram(t, KZ)
    x = mp_inverse_column(t)
    n = len(x)
    p, acc = [], mp.mpf(0)
    for r in range(n):
        acc += x[r] * x[r] - (x[n - r] * x[n - r] if r else 0)
        p.append(acc / x[0])
    return G, p


def dense(t, KZ):
    n = len(t)
    T = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            T[i, j] = t[abs(i - j)]
    Ti = mp.inverse(T)
    M = mp.matrix([[mp.mpf(float(v)) for v in row] for row in KZ])
    G = M.T * (Ti * M)
    c = KZ.shape[1]
    return [[G[a, b] for b in range(c)] for a in range(c)], [Ti[i, i] for i in range(n)]


def run(job):
    case, cache = job
    name, n = case["name"], case["n"]
    path = cache and os.path.join(cache, f"post_{name}.json")
    if path and os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    mp.mp.dps = WORK
    t0 = time.time()
    cols = pc.golden_cols(n)
    s = pc.off_grid_points(n)
    q = len(s)
    KZ = np.concatenate([pc.lorentz_columns(n, s), tc.rhs_columns(n, cols)], axis=1)
    t = mpf_list(tc.hex_column(case))
    G, p = structured(t, KZ)
    method = "recursion"
    if n <= 128:
        want = dense(t, KZ)
        d = [mp.nstr(worst(G, want[0]), 3), mp.nstr(worst(p, want[1]), 3)]
        print(f"self-check {name}: the O(n^2) routes against the dense inverse: Gram {d[0]}, p {d[1]}", flush=True)
        assert all(mp.mpf(v) <= mp.mpf("1e-50") for v in d), (name, d)
        G, p = want
        method = "dense"
    out = dict(name=name, n=n, cols=cols, q=q, s=[float(v) for v in s], method=method,
               quad=[float(G[j][j]) for j in range(q)], cross=[[float(G[j][q + b]) for b in range(cols)] for j in range(q)],
               cov=[[float(G[a][b]) for b in range(q)] for a in range(q)], p=[float(v) for v in p])
    print(f"{name}: {time.time() - t0:.0f} s", flush=True)
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
        for k in ("quad", "cross", "cov", "p"):
            arrays[r["name"] + "/" + k] = np.array(r.pop(k))
    np.savez_compressed(os.path.join(HERE, "toeplitz_post.npz"), **arrays)
    with open(os.path.join(HERE, "toeplitz_post.json"), "w") as f:
        json.dump(dict(method=f"mpmath, answers held to {DIGITS} digits (computed at {WORK}) on the Toeplitz matrices of the fp64 columns t "
                              "(t_hex of toeplitz.json / toeplitz_classes.json), rounded to fp64 at the end; n <= 128: the dense inverse; "
                              "above: the Schur recursion with the forward substitution, and Levinson's recursion with the "
                              "Gohberg-Semencul prefix for p, checked against the dense answers at n <= 128 to 1e-50 "
                              "(make_golden_toeplitz_post.py)",
                       digits=DIGITS, inputs="K = toeplitz_post_cases.lorentz_columns(n, s), Z = toeplitz_cases.rhs_columns(n, cols); quad, cross, "
                                             "cov and p are in toeplitz_post.npz under <name>/quad, /cross, /cov and /p",
                       cases=done), f)


if __name__ == "__main__":
    main()
