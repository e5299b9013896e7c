"""Leave-group-out on one device: milliseconds by phase, host-to-host time, TF/s of the Gram and of the block factorisation, and
backend='cpu' on the same factor beside them.  One process, one JSON line per (n, layout).

    python tools/gpu_kfold_rates.py [--sizes 2048 8192] [--curves 3] [--reps 3] [--no-cpu] [--out FILE]

The factor is numpy's Cholesky factor of the RBF at 0.75 grid spacings with a nugget of 1e-6 (section 15's).  The flop counts
are the arithmetic the kernels execute on their tiles after the skipped zeros are taken out, counted on the host from the groups:
Gram 2 * 64 * 64 * (N - kbeg) per tile of the upper block triangle; factorisation g_b^3 / 3 per diagonal block plus the panel
and trailing products of every step; `useful` is the closed count sum_G (n g^2 + 2/3 g^3) without any skipping or padding.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import gsum_amd as gm  # noqa: E402
from gsum_amd.loo import LooFactor, normalise_folds  # noqa: E402

PEAK_TFLOPS = 78.6
BLOCK, TILE, KC = 128, 64, 16


def layouts(n):
    return {
        "folds=5": 5,
        "folds=10": 10,
        "blocks of 64": np.arange(n) // 64,
        "interleaved 5": gm.make_folds(n, 5, "interleaved"),
    }


def executed_flops(n, fold_ptr, fold_idx):
    """(gram, factor, useful) flops of one call."""
    N = -(-n // BLOCK) * BLOCK
    gram = factor = useful = 0.0
    for q in range(len(fold_ptr) - 1):
        idx = np.sort(fold_idx[fold_ptr[q]:fold_ptr[q + 1]])
        g = idx.size
        gp = -(-g // BLOCK) * BLOCK
        useful += n * g * g + 2.0 / 3.0 * g ** 3
        first = np.full(gp // TILE, N - KC)
        live = np.arange(0, g, TILE)
        first[:live.size] = idx[live] // KC * KC
        for t in range(gp // TILE):                                 # tiles (m, t) with m <= t start at tile t's first index
            gram += (t + 1) * 2.0 * TILE * TILE * (N - first[t])
        for b in range(gp // BLOCK):
            rest = gp - (b + 1) * BLOCK
            factor += BLOCK ** 3 / 3.0 + 2.0 * BLOCK * BLOCK * rest * 0.75      # diagonal block; panel (lower-triangular inverse)
            tn = rest // TILE
            factor += tn * (tn + 1) / 2 * 2.0 * TILE * TILE * BLOCK             # trailing update, upper block triangle
    return gram, factor, useful


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--curves", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None
    for n in args.sizes:
        x = np.arange(n, dtype=float)
        K = np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2 / 0.75 ** 2) + 1e-6 * np.eye(n)
        L = np.linalg.cholesky(K)
        del K
        Y = np.random.RandomState(0).standard_normal((n, args.curves))
        dev = LooFactor(L, backend="hip")
        cpu = None if args.no_cpu else LooFactor(L, backend="cpu")
        try:
            for name, folds in layouts(n).items():
                fold_ptr, fold_idx, _ = normalise_folds(folds, n)
                gram, factor, useful = executed_flops(n, fold_ptr, fold_idx)
                dev.folds(Y, folds)                                 # warm-up
                dev.fold_times(reset=True)
                dev.times(reset=True)
                walls = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    res = dev.folds(Y, folds)
                    walls.append((time.perf_counter() - t0) * 1e3)
                ms = {k: v / args.reps for k, v in dev.fold_times().items()}
                solve = {k: v / args.reps for k, v in dev.times().items() if k in ("h2d", "solve")}
                line = {
                    "n": n, "layout": name, "n_folds": int(len(fold_ptr) - 1), "curves": args.curves, "reps": args.reps,
                    "device_ms_by_phase": ms, "solve_ms": solve, "device_ms": sum(ms.values()) + sum(solve.values()),
                    "wall_ms_min": min(walls), "wall_ms_mean": float(np.mean(walls)),
                    "gram_gflop": gram / 1e9, "factor_gflop": factor / 1e9, "useful_gflop": useful / 1e9,
                    "gram_tflops": gram / (ms["gram"] * 1e-3) / 1e12, "factor_tflops": factor / (ms["factor"] * 1e-3) / 1e12,
                    "gram_share_of_peak": gram / (ms["gram"] * 1e-3) / 1e12 / PEAK_TFLOPS,
                    "bounding_phase": max(ms, key=ms.get),
                }
                if cpu is not None:
                    t0 = time.perf_counter()
                    ref = cpu.folds(Y, folds)
                    line["cpu_wall_ms"] = (time.perf_counter() - t0) * 1e3
                    line["max_rel_gap_var"] = float(np.max(np.abs(res.var - ref.var) / ref.var))
                    line["max_rel_gap_mean"] = float(np.max(np.abs(res.mean - ref.mean)) / np.max(np.abs(ref.mean)))
                text = json.dumps(line)
                print(text, flush=True)
                if out:
                    out.write(text + "\n")
                    out.flush()
        finally:
            dev.free()
            if cpu is not None:
                cpu.free()
    if out:
        out.close()


if __name__ == "__main__":
    main()
