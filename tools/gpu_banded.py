"""The banded likelihood path on one device beside the other routes: the 64 x 64 (length scale, ratio) surface at
n = 2048 and n = 8192 through ``structure="banded"``, dense ``mode="full"``, dense ``mode="reuse"`` and ``structure="toeplitz"`` with
``toeplitz_method="blocked"`` in one session, and one matrix with five right-hand sides on sorted non-uniform points at n = 8192,
65 536 and 1 048 576 for b = 77 and b = the library's widest.  Writes one JSON file.

    python tools/gpu_banded.py [--out profiles/banded_rates.json] [--grid 64] [--reps 2] [--timeout 300]

Every step runs in a child process of its own under its own time limit (``--step NAME`` is what the child runs); the first step that
fails or runs out of time ends the run, and what was measured until then is still written.

Inputs of the surface: X = 0.1 * arange(n), RBF with length scales linspace(0.05, 0.2, grid), ratios linspace(0.3, 0.7, grid), five
curves (sets of c = 6 columns), nugget 1e-10.  Rates are evaluations (grid points) per second of host-to-host wall time, the best of
``reps`` after one warm-up call; the device milliseconds of the library's phases are beside them.  Inputs of the single matrix: a
diagonally dominant band of the given width (the factorisation's cost does not depend on the entries), wall time host arrays to host
result, and the phases.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SURFACE_SIZES = (2048, 8192)
SINGLE_SIZES = (8192, 65536, 1048576)
ROUTES = ("banded", "full", "reuse", "toeplitz")


def steps():
    return [f"surface:{n}:{route}" for n in SURFACE_SIZES for route in ROUTES] + [f"single:{n}:{b}" for n in SINGLE_SIZES for b in ("77", "widest")]


def surface(n, route, grid, reps):
    from sklearn.gaussian_process.kernels import RBF
    import gsum_amd as gm
    r = 5
    X = 0.1 * np.arange(n)[:, None]
    y = gm.partials(np.random.RandomState(0).randn(n, r), ratio=0.5, ref=1.0, orders=np.arange(r))
    gp = gm.TruncationGP(kernel=RBF(0.2), ratio=0.5, ref=1.0, center=0, disp=0, df=1, scale=1, optimizer=None)
    gp.X_train_, gp.y_train_, gp.orders_ = X, y, np.arange(r)
    thetas = [np.log([v]) for v in np.linspace(0.05, 0.2, grid)]
    ratios = list(np.linspace(0.3, 0.7, grid))
    kw = {"banded": dict(structure="banded"), "toeplitz": dict(structure="toeplitz", toeplitz_method="blocked")}.get(route, dict(mode=route))
    gp.log_marginal_likelihood_grid(thetas[:2], ratios[:2], **kw)                  # warm-up: libraries, buffers, clocks
    handle = None
    if route == "banded":
        from gsum_amd import _band_lib
        handle = _band_lib.default_handle(0)
        handle.times(reset=True)
    walls, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = gp.log_marginal_likelihood_grid(thetas, ratios, **kw)
        walls.append(time.perf_counter() - t0)
    res = dict(n=n, route=route, grid=[grid, grid], curves=r, reps=reps, wall_s=walls, evals_per_s=grid * grid / min(walls),
               finite=int(np.isfinite(out).sum()), argmax=[int(v) for v in np.unravel_index(np.argmax(out), out.shape)], max=float(np.max(out)))
    if handle is not None:
        res["device_ms_by_phase_per_call"] = {k: v / reps for k, v in handle.times().items()}
    return res


def single(n, b, reps):
    import gsum_amd as gm
    from gsum_amd import _band_lib
    b = _band_lib.max_halfwidth() if b == "widest" else int(b)
    rng = np.random.RandomState(2)
    AB = np.empty((b + 1, n))
    AB[1:] = 0.3 * rng.standard_normal((b, n))
    AB[0] = 2.0 + 0.6 * b + rng.random_sample(n)
    Z = rng.standard_normal((n, 5))
    h = _band_lib.default_handle(0)
    gm.banded_gram(AB[:, :4096], Z[:4096])                                         # warm-up
    h.times(reset=True)
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        G, sld, info = gm.banded_gram(AB, Z)
        walls.append(time.perf_counter() - t0)
    assert info == 0 and np.all(np.isfinite(G))
    return dict(n=n, b=b, columns=5, reps=reps, wall_s=walls, device_ms_by_phase_per_call={k: v / reps for k, v in h.times().items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "banded_rates.json"))
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--step", default=None)
    ap.add_argument("--only", default=None, help="run the steps that start with this prefix")
    args = ap.parse_args()
    if args.step:
        kind, n, rest = args.step.split(":")
        res = surface(int(n), rest, args.grid, args.reps) if kind == "surface" else single(int(n), rest, args.reps)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    results, failed = {}, None
    for step in steps():
        if args.only and not step.startswith(args.only):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--grid", str(args.grid), "--reps", str(args.reps)]
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
    for n in SURFACE_SIZES:
        rate = {route: results.get(f"surface:{n}:{route}", {}).get("evals_per_s") for route in ROUTES}
        if all(rate.values()):
            results[f"ratio:{n}"] = {f"banded_over_{route}": rate["banded"] / rate[route] for route in ROUTES[1:]}
    if failed:
        results["stopped_at"] = failed
        print("stopped:", failed, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1, sort_keys=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
