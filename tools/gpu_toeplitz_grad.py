"""The Toeplitz gradient path on one device: the device milliseconds of ``toeplitz_grad`` by phase for one first
column at n = 2048, 4096 and 8192 (c = 4, one derivative column), and one ``fit`` with four restarts at n = 2048 through
``structure="toeplitz"`` and through the dense route.  Writes one JSON file.

    python tools/gpu_toeplitz_grad.py [--out profiles/toeplitz_grad_<date>.json] [--reps 3] [--timeout 300]

Every step runs in a child process of its own under its own time limit (``--step NAME`` is what the child runs); the first step that
fails or runs out of time ends the run, and what was measured until then is still written.

Inputs of the fit: X = 0.1 * arange(2048), three curves of seeded normals drawn through the Cholesky factor of RBF(0.3) + 1e-6 I at the
first 256 points and tiled, kernel RBF(0.2) with a free length scale plus a fixed WhiteKernel(1e-6), n_restarts_optimizer=4,
random_state=0.  Wall times are host to host, the second of two fits (the first warms libraries, buffers and clocks).
"""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNEL_SIZES = (2048, 4096, 8192)
FIT_N = 2048
ROUTES = ("toeplitz", "dense")


def steps():
    return [f"kernel:{n}" for n in KERNEL_SIZES] + [f"fit:{route}" for route in ROUTES]


def kernel(n, reps):
    from gsum_amd import _toep_lib
    h = _toep_lib.default_handle(0)
    x = 0.1 * np.arange(n)
    t = np.exp(-0.5 * (x / 0.1) ** 2)
    dt = (t * (x / 0.1) ** 2)[None, None]
    t[0] += 1e-10
    Z = np.random.RandomState(1).randn(n, 4)
    h.grad(t[None], dt, Z, 1)
    h.gram(t[None], Z, 1)
    h.grad_times(reset=True)
    h.times(reset=True)
    for _ in range(reps):
        out = h.grad(t[None], dt, Z, 1)
        h.gram(t[None], Z, 1)
    assert out[2][0] == 0
    return dict(n=n, c=4, P=1, reps=reps, grad_ms_by_phase={k: v / reps for k, v in h.grad_times().items()},
                value_ms_by_phase={k: v / reps for k, v in h.times().items()})


def fit(route):
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel
    import gsum_amd as gm
    n = FIT_N
    X = 0.1 * np.arange(n)[:, None]
    blk = 256
    L = np.linalg.cholesky(RBF(0.3)(X[:blk]) + 1e-6 * np.eye(blk))
    y = np.tile(L @ np.random.RandomState(0).randn(blk, 3), (n // blk, 1))
    walls, gp = [], None
    for _ in range(2):
        gp = gm.ConjugateGaussianProcess(kernel=RBF(0.2) + WhiteKernel(1e-6, noise_level_bounds="fixed"), n_restarts_optimizer=4, random_state=0)
        t0 = time.perf_counter()
        gp.fit(X, y, structure="toeplitz" if route == "toeplitz" else None)
        walls.append(time.perf_counter() - t0)
    return dict(n=n, route=route, restarts=4, wall_s=walls, theta=[float(v) for v in gp.kernel_.theta], value=float(gp.log_marginal_likelihood_value_))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", f"toeplitz_grad_{datetime.date.today().isoformat()}.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    if args.step:
        kind, arg = args.step.split(":")
        res = kernel(int(arg), args.reps) if kind == "kernel" else fit(arg)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    results, failed = {}, None
    for step in steps():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            failed = f"{step}: no result within {args.timeout} s"
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            failed = f"{step}: exit status {p.returncode}: {p.stderr[-2000:]}"
            break
        results[step] = json.loads(lines[-1][7:])
        print(step, json.dumps(results[step]), flush=True)
    if all(f"fit:{r}" in results for r in ROUTES):
        results["fit:toeplitz_over_dense_wall"] = results["fit:toeplitz"]["wall_s"][-1] / results["fit:dense"]["wall_s"][-1]
    if failed:
        results["stopped_at"] = failed
        print("stopped:", failed, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1, sort_keys=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
