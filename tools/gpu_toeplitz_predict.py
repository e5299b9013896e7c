"""The posterior on the Toeplitz route on one device: ``predict(return_std=True)`` and ``predict(return_cov=True)``
at n = 2048 and 8192 with q = 256 and 2048 new points, ``loo`` at both sizes, and ``fit`` with the device memory it leaves held, each
through the structured route (``fit(structure="toeplitz", dense_factor=False)``) and through the dense factor on the same kernel.
Writes one JSON file.

    python tools/gpu_toeplitz_predict.py [--out profiles/toeplitz_predict_<date>.json] [--timeout 300]

Every step runs in a child process of its own under its own time limit (``--step NAME`` is what the child runs); the first step that
fails or runs out of time ends the run, and what was measured until then is still written.

Inputs: X = linspace(0, 1, n), three curves of seeded normals, kernel Matern(0.2, nu=0.5) with a free length scale plus a fixed
WhiteKernel(1e-6); the new points are linspace(-0.05, 1.05, q).  predict and loo run on a process fitted with optimizer=None; wall times
are host arrays to host result, the best of two calls after one warm-up, and the structured route's device milliseconds by phase
(``gsum_toep_post_times``) are those of the last call.  fit runs the optimiser once from the kernel's own start; the memory figure is
the drop of hipMemGetInfo's free bytes from before the first fit to after the second.
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

SIZES = (2048, 8192)
NEW_POINTS = (256, 2048)
ROUTES = ("toeplitz", "dense")


def steps():
    out = [f"predict:{route}:{n}:{q}:{what}" for n in SIZES for q in NEW_POINTS for what in ("std", "cov") for route in ROUTES]
    out += [f"loo:{route}:{n}" for n in SIZES for route in ROUTES]
    return out + [f"fit:{route}:{n}" for n in SIZES for route in ROUTES]


def process(n, optimizer):
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    import gsum_amd as gm
    X = np.linspace(0, 1, n)[:, None]
    y = np.random.RandomState(1).randn(n, 3)
    return gm.ConjugateGaussianProcess(kernel=Matern(0.2, nu=0.5) + WhiteKernel(1e-6, noise_level_bounds="fixed"), optimizer=optimizer), X, y


def best_of_two(call):
    call()
    walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    return min(walls)


def post_phases():
    from gsum_amd import _toep_lib
    return _toep_lib.default_handle(0)


def predict(route, n, q, what):
    gp, X, y = process(n, None)
    gp.fit(X, y, structure="toeplitz", dense_factor=route == "dense")
    Xs = np.linspace(-0.05, 1.05, q)[:, None]
    kw = dict(return_std=True) if what == "std" else dict(return_cov=True)
    h = post_phases() if route == "toeplitz" else None

    def call():
        if h is not None:
            h.post_times(reset=True)
        gp.predict(Xs, **kw)

    out = dict(route=route, n=n, q=q, what=what, wall_s=best_of_two(call))
    if h is not None:
        out["device_ms_by_phase"] = h.post_times()
    return out


def loo(route, n):
    gp, X, y = process(n, None)
    gp.fit(X, y, structure="toeplitz", dense_factor=route == "dense")
    h = post_phases() if route == "toeplitz" else None

    def call():
        if h is not None:
            h.post_times(reset=True)
        gp.loo()

    out = dict(route=route, n=n, curves=3, wall_s=best_of_two(call))
    if h is not None:
        out["device_ms_by_phase"] = h.post_times()
    return out


def fit(route, n):
    import torch
    torch.cuda.init()
    free0 = torch.cuda.mem_get_info(0)[0]                              # hipMemGetInfo
    walls, gp = [], None
    for _ in range(2):
        gp, X, y = process(n, "fmin_l_bfgs_b")
        t0 = time.perf_counter()
        gp.fit(X, y, structure="toeplitz", dense_factor=route == "dense")
        walls.append(time.perf_counter() - t0)
    held = free0 - torch.cuda.mem_get_info(0)[0]
    return dict(route=route, n=n, wall_s=walls, device_bytes_held=int(held), theta=[float(v) for v in gp.kernel_.theta],
                value=float(gp.log_marginal_likelihood_value_))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", f"toeplitz_predict_{datetime.date.today().isoformat()}.json"))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    if args.step:
        kind, route, *rest = args.step.split(":")
        res = (predict(route, int(rest[0]), int(rest[1]), rest[2]) if kind == "predict" else
               loo(route, int(rest[0])) if kind == "loo" else fit(route, int(rest[0])))
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    results, failed = {}, None
    for step in steps():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step]
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
    for step in [s for s in results if ":toeplitz:" in s]:
        other = step.replace(":toeplitz:", ":dense:")
        if other in results:
            a, b = results[step]["wall_s"], results[other]["wall_s"]
            results[step.replace(":toeplitz:", ":toeplitz_over_dense_wall:")] = (a[-1] / b[-1]) if isinstance(a, list) else a / b
    if failed:
        results["stopped_at"] = failed
        print("stopped:", failed, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:                                     # one step per line
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(results[k], sort_keys=True)}" for k in sorted(results)) + "\n}\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
