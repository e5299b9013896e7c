#!/usr/bin/env python3
"""Rates of the diagnostic square roots: device pstrf and potrf at n = 2048 / 8192 / 16384, sqrt_errors for
k = 1000 at n = 8192 (n^2 k flops), and scipy's dpstrf on the host's CPUs at 2048 / 8192 in the same run.  One JSON line.

    python tools/gpu_diagnostic_rates.py [--reps 3]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scipy.linalg.lapack import dpstrf  # noqa: E402
from sklearn.gaussian_process.kernels import Matern  # noqa: E402

import gsum_amd as gm  # noqa: E402


def spd(n):
    X = np.random.RandomState(n).uniform(0, 1, (n, 2))
    return Matern(0.3, nu=2.5)(X) + 1e-3 * np.eye(n)


def device_ms(ctx, A, pivot, reps):
    best = []
    for _ in range(reps):
        M = ctx.upload(A)
        t0 = time.perf_counter()
        info = ctx.pstrf(M)[0] if pivot else ctx.potrf(M)
        best.append((time.perf_counter() - t0) * 1e3)
        M.free()
        assert info == 0, info
    return min(best)


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    ctx = gm.default_context()
    out = {"tool": "gpu_diagnostic_rates", "reps": reps}
    for n in (2048, 8192, 16384):
        A = spd(n)
        device_ms(ctx, A, True, 1)                                       # warm-up (scratch allocation, code objects)
        out[f"pstrf_ms_{n}"] = round(device_ms(ctx, A, True, reps), 3)
        out[f"potrf_ms_{n}"] = round(device_ms(ctx, A, False, reps), 3)
    n, k = 8192, 1000
    A = spd(n)
    Y = np.random.RandomState(1).standard_normal((n, k))
    F = ctx.upload(A)
    ctx.sqrt_errors(F, Y[:, :1], pivot=False)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.sqrt_errors(F, Y, pivot=False, errors=True, md2=True)
        ts.append((time.perf_counter() - t0) * 1e3)
    F.free()
    out["sqrt_errors_ms_8192_k1000"] = round(min(ts), 3)
    out["sqrt_errors_tflops_8192_k1000"] = round(n * n * k / (min(ts) * 1e-3) / 1e12, 3)
    for n in (2048, 8192):
        A = spd(n)
        t0 = time.perf_counter()
        dpstrf(A, tol=-1.0, lower=1)
        out[f"host_dpstrf_ms_{n}"] = round((time.perf_counter() - t0) * 1e3, 1)
    out["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
