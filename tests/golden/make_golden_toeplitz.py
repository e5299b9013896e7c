#!/usr/bin/env python3
"""Known answers of the Toeplitz likelihood path -> tests/golden/toeplitz.json.

"ill": ill-conditioned first columns t (smooth kernels on linspace(0, 1, n), nugget 1e-10).  Truth is a Cholesky factorisation, a
forward substitution and the Gram matrix in mpmath at 60 digits of the symmetric Toeplitz matrix of the fp64 t: G = Z^T T^-1 Z and
sum_j log L_jj, rounded to fp64.  The file holds G, sum_log_diag and the recipe of the inputs: the kernel, the grid, the columns of Z
(tests/toeplitz_cases.py: rhs_columns) and the bits of t themselves (hex), because an exp that differs in its last bit between two
libm builds would move these answers by far more than the bounds of the tests.

"large": the S2 / S3 inputs of large_lml.json (0.1 * arange(n), RBF(0.2), nugget 1e-10, white-noise coefficients) at n = 512 and
2048: the log likelihood of the Toeplitz matrix of t, made the way make_truth.py makes large_truth.json (80-bit long double
factorisation in oracle/truth_ld.c, numpy.longdouble algebra).  Needs mpmath, gcc, numpy and scikit-learn (no reference import).

    python tests/golden/make_golden_toeplitz.py
"""
import json
import os
import sys

import mpmath as mp
import numpy as np
from scipy.linalg import toeplitz
from sklearn.gaussian_process.kernels import RBF, Matern, WhiteKernel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from oracle import gsum_oracle as orc  # noqa: E402
from toeplitz_cases import rhs_columns  # noqa: E402
import make_truth  # noqa: E402

mp.mp.dps = 60
NUGGET = 1e-10
ILL = [("rbf_n64", "RBF(0.2)", 64), ("rbf_n128", "RBF(0.2)", 128), ("matern52_n64", "Matern(0.2, nu=2.5)", 64),
       ("matern52_n128", "Matern(0.2, nu=2.5)", 128), ("rbf_white_n128", "RBF(0.2) + WhiteKernel(1e-8)", 128)]


def first_column(kernel, X, nugget):
    t = kernel(X, X[:1])[:, 0]
    t[0] = kernel.diag(X[:1])[0] + nugget
    return t


def mp_gram(t, Z):
    n, c = Z.shape
    tm = [mp.mpf(float(v)) for v in t]
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for j in range(n):
        Lj = L[j]
        d = mp.sqrt(tm[0] - mp.fsum(v * v for v in Lj[:j]))
        Lj[j] = d
        for i in range(j + 1, n):
            Li = L[i]
            Li[j] = (tm[i - j] - mp.fsum(Li[k] * Lj[k] for k in range(j))) / d
    Y = [[mp.mpf(0)] * c for _ in range(n)]
    for i in range(n):
        for a in range(c):
            Y[i][a] = (mp.mpf(float(Z[i, a])) - mp.fsum(L[i][k] * Y[k][a] for k in range(i))) / L[i][i]
    G = [[float(mp.fsum(Y[k][a] * Y[k][b] for k in range(n))) for b in range(c)] for a in range(c)]
    return G, float(mp.fsum(mp.log(L[j][j]) for j in range(n)))


def main():
    env = dict(RBF=RBF, Matern=Matern, WhiteKernel=WhiteKernel)
    ill = []
    for name, expr, n in ILL:
        X = np.linspace(0, 1, n)[:, None]
        t = first_column(eval(expr, {"__builtins__": {}}, env), X, NUGGET)
        G, sld = mp_gram(t, rhs_columns(n, 4))
        ill.append(dict(name=name, kernel=expr, n=n, grid="linspace(0, 1, n)", nugget=NUGGET, cols=4, t_hex=[float(v).hex() for v in t],
                        G=G, sum_log_diag=sld))
        print(name, sld, flush=True)
    lib = make_truth.load_lib()
    large = []
    for n, r in ((512, 4), (2048, 4)):
        X = 0.1 * np.arange(n)[:, None]
        t = first_column(RBF(0.2), X, NUGGET)
        T = np.ascontiguousarray(toeplitz(t))
        orders = np.arange(r)
        y = orc.partials(np.random.RandomState(0).randn(n, r), ratio=0.5, ref=1.0, orders=orders)
        for q in (0.5, 0.45):
            c = orc.coefficients(y, q * np.ones(n), np.ones(n), orders)
            jac = np.sum(r * np.log(np.abs(np.ones(n))) + np.sum(orders) * np.log(np.abs(q * np.ones(n))))
            lml, _, sld = make_truth.truth_lml(lib, T, c, jac)
            large.append(dict(n=n, r=r, seed=0, ratio=q, lml_truth=repr(lml), lml_truth_f64=float(lml), sum_log_diag_truth=float(sld)))
            print(large[-1], flush=True)
        large[-1]["t_hex"] = large[-2]["t_hex"] = [float(v).hex() for v in t]
    with open(os.path.join(HERE, "toeplitz.json"), "w") as f:
        json.dump(dict(method="ill: mpmath at 60 digits on the Toeplitz matrix of the fp64 first column t (t_hex); large: 80-bit long double "
                              "(oracle/truth_ld.c) + numpy.longdouble algebra on the Toeplitz matrix of t, inputs as large_lml.json",
                       ill=ill, large=large), f)


if __name__ == "__main__":
    main()
