#!/usr/bin/env python3
"""Variogram rates on the device: compute() wall time (warmed up, ends in the library's synchronise) for N in {500, 1000, 2000,
4000}, d = 1, 4 curves, GraphicalDiagnostic's bin rule (nbins = ceil(P^(1/3)), P = N (N - 1) / 2).

    python tools/vario_rates.py [--cpu]          wall times, terms/s, share of the FP64 vector peak
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/vario_rates.py --once     (kernel times: a run of its own)

Terms: sum over bins of m_b^2 per curve (the reference's count); the kernel evaluates m_b (m_b + 1) / 2 of them (t(p,q) = t(q,p)).
FLOPs per evaluated term and curve, counted from the kernel's source: 4 adds (rho's numerator), 1 division (about 10 FP64 ops as
lowered), 1 multiply (rho^2), the two polynomial branches (20 FMA for x < 1/2; 2 x 19 FMA, a log of about 25 ops and 5 more for
x >= 1/2; a wave with lanes on both sides runs both) and 3 for the clamp and the sum: ~ 100.  Peak: 78.6 TF/s FP64 vector.
--cpu adds backend='cpu' times at N = 120 and 250 (for scale).
"""
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import gsum_amd as gm  # noqa: E402

FLOPS_PER_TERM = 100
PEAK = 78.6e12


def problem(N, nc=4, seed=0):
    rng = np.random.RandomState(seed)
    X = np.sort(rng.uniform(0, 1, N))[:, None]
    z = rng.standard_normal((nc, N)).cumsum(axis=1) / np.sqrt(N)
    P = N * (N - 1) / 2
    bounds = np.linspace(0, np.max(np.linalg.norm(X, axis=-1)), int(np.ceil(P ** (1. / 3))))
    return X, z, bounds


def main():
    once = "--once" in sys.argv
    sizes = (500, 1000, 2000) if once else (500, 1000, 2000, 4000)
    for N in sizes:
        X, z, bounds = problem(N)
        t0 = time.perf_counter()
        v = gm.VariogramFourthRoot(X, z, bounds, backend="hip")
        t_create = time.perf_counter() - t0
        v.compute()                                                   # warm-up
        reps = 1 if once else 3
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            v.compute()
            ts.append(time.perf_counter() - t0)
        m = v.bin_counts.astype(float)
        full_terms = float(np.sum(m * m)) * v.Ncurves
        eval_terms = float(np.sum(m * (m + 1) / 2)) * v.Ncurves
        t = min(ts)
        print(f"N={N:5d} bins={v.Nb:4d} create={t_create:.3f}s compute={t:.3f}s (of {['%.3f' % x for x in ts]}) "
              f"terms={full_terms:.3e} evaluated={eval_terms:.3e} terms/s={full_terms / t:.3e} "
              f"evaluated/s={eval_terms / t:.3e} fp64_share={eval_terms * FLOPS_PER_TERM / t / PEAK:.1%}", flush=True)
        v.close()
    if "--cpu" in sys.argv:
        for N in (120, 250):
            X, z, bounds = problem(N)
            t0 = time.perf_counter()
            v = gm.VariogramFourthRoot(X, z, bounds, backend="cpu")
            v.compute()
            print(f"cpu N={N}: construct + compute {time.perf_counter() - t0:.2f} s", flush=True)


if __name__ == "__main__":
    main()
