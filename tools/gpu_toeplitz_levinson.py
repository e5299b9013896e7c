"""The tiled Levinson replay of the Toeplitz path on one device.  Writes one JSON file.

    python tools/gpu_toeplitz_levinson.py [--out profiles/toeplitz_levinson_<date>.json] [--timeout 300] [--only TEXT]

Part 1, where both methods exist: ``toeplitz_grad`` of one ARFIMA(0, 0.4, 0) first column with c = 4 right-hand sides and P = 1
derivative column at n = 2048, 4096 and 8192 through ``method="columns"`` and ``"blocked"``: wall time and the device milliseconds by
phase (the ``levinson`` phase of either clock is k_levinson against the tiles).

Part 2, beyond the default method's limit: the same through ``method="blocked"`` at n = 16384, 65536 and 262144, and
``toeplitz_inverse_column`` alone at 262144 and 1048576.  The time limit of the last is sized from the 262144 run, times 16 for the n^2
growth and times 2 for margin; if the projection (times 16) exceeds ten minutes the projection is recorded and the run skipped.

Part 3: one ``fit`` with the default optimiser, ``toeplitz_method="blocked"`` and ``toeplitz_grad_method="blocked"`` without the dense
factor at n = 16385, timed once, with its number of objective evaluations.

Every step runs in a child process of its own under its own time limit (``--step NAME`` is what the child runs); the first step that
fails or runs out of time ends the run, and what was measured until then is still written.  Wall times are host arrays to host result,
one warm-up and then two calls (one from n = 65536 on): the best and the spread; the device milliseconds are those of the last call."""
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

BOTH = (2048, 4096, 8192)
BEYOND = (16384, 65536, 262144)
COLUMN_FROM, COLUMN_AT = 262144, 1048576
FIT_N = 16385
K_LEVINSON_MS_RECORDED = {2048: 1.8, 4096: 7.0, 8192: 24.8}


def steps():
    out = [f"grad:{method}:{n}" for n in BOTH for method in ("columns", "blocked")]
    out += [f"grad:blocked:{n}" for n in BEYOND]
    return out + [f"column:blocked:{COLUMN_FROM}", f"column:blocked:{COLUMN_AT}", f"fit:blocked:{FIT_N}"]


def arfima_column(n, d):
    t = [1.0]
    for k in range(1, n):
        t.append(t[-1] * (k - 1 + d) / (k - d))
    return np.array(t)


def timed(call, n):
    call()
    walls = []
    for _ in range(2 if n < 65536 else 1):
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    return dict(wall_s=min(walls), wall_spread_s=max(walls) - min(walls), calls_timed=len(walls))


def clock(h, method):
    ms = (h.levinson_times if method == "blocked" else h.grad_times)()
    return dict(device_ms_by_phase=ms, device_ms=sum(ms.values()), levinson_ms=ms["levinson"])


def reset(h):
    h.grad_times(reset=True)
    h.levinson_times(reset=True)


def grad(method, n):
    import gsum_amd as gm
    from gsum_amd import _toep_lib
    h = _toep_lib.default_handle(0)
    t, Z = arfima_column(n, 0.4), np.random.RandomState(0).randn(n, 4)
    dt = (np.arange(n) * t)[None]
    got = {}

    def call():
        reset(h)
        got["r"] = gm.toeplitz_grad(t, dt, Z, 1, method=method)
        assert got["r"][2] == 0

    out = dict(method=method, n=n, cols=4, P=1, **timed(call, n))
    out.update(clock(h, method))
    out["finite"] = bool(all(np.isfinite(a).all() for a in got["r"]))
    if n in K_LEVINSON_MS_RECORDED:
        out["k_levinson_ms_recorded_in_section_19"] = K_LEVINSON_MS_RECORDED[n]
    return out


def column(n):
    import gsum_amd as gm
    from gsum_amd import _toep_lib
    h = _toep_lib.default_handle(0)
    t = arfima_column(n, 0.4)
    reset(h)
    t0 = time.perf_counter()
    x, info = gm.toeplitz_inverse_column(t, method="blocked")
    wall = time.perf_counter() - t0
    assert info == 0
    out = dict(method="blocked", n=n, wall_s=wall, calls_timed=1, warm_up=False, finite=bool(np.isfinite(x).all()), x0=float(x[0]))
    out.update(clock(h, "blocked"))
    return out


def fit(n):
    import gsum_amd as gm
    from gsum_amd import toeplitz as tz
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    e = np.random.RandomState(1).randn(n, 2)
    phi = np.exp(-1.0 / ((n - 1) * 0.1))                                # exact draws of the Matern-1/2 process with length scale 0.1
    y = np.empty((n, 2))
    y[0] = e[0]
    for i in range(1, n):
        y[i] = phi * y[i - 1] + np.sqrt(1 - phi * phi) * e[i]
    X = np.linspace(0, 1, n)[:, None]
    gp = gm.ConjugateGaussianProcess(kernel=Matern(0.2, nu=0.5) + WhiteKernel(1e-6, noise_level_bounds="fixed"), center=0.1, disp=1.5, df=2, scale=0.7)
    calls, real = [0], tz.toeplitz_grad

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    tz.toeplitz_grad = counted
    t0 = time.perf_counter()
    gp.fit(X, y, structure="toeplitz", dense_factor=False, toeplitz_method="blocked", toeplitz_grad_method="blocked")
    wall = time.perf_counter() - t0
    tz.toeplitz_grad = real
    from gsum_amd import _toep_lib
    return dict(n=n, wall_s=wall, calls_timed=1, warm_up=False, objective_evaluations=calls[0], length_scale=float(np.exp(gp.kernel_.theta)[0]),
                log_marginal_likelihood=float(gp.log_marginal_likelihood_value_), **clock(_toep_lib.default_handle(0), "blocked"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", f"toeplitz_levinson_{datetime.date.today().isoformat()}.json"))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--only", default=None, help="run the steps that contain this text")
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    if args.step:
        kind, method, n = args.step.split(":")
        res = grad(method, int(n)) if kind == "grad" else column(int(n)) if kind == "column" else fit(int(n))
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    results, failed = {}, None
    for step in [s for s in steps() if args.only is None or args.only in s]:
        limit = args.timeout
        if step == f"column:blocked:{COLUMN_AT}":
            base = results.get(f"column:blocked:{COLUMN_FROM}")
            if base is None:
                continue
            projected = 16 * base["wall_s"]
            if projected > 600:
                results[step] = dict(skipped=True, projected_wall_s=projected, projected_from=COLUMN_FROM)
                continue
            limit = int(2 * projected) + 60                              # the process start, the imports and the column itself on top
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            failed = f"{step}: no result within {limit} s"
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            failed = f"{step}: exit status {p.returncode}: {p.stderr[-2000:]}"
            break
        results[step] = dict(json.loads(lines[-1][7:]), time_limit_s=limit)
        print(step, json.dumps(results[step]), flush=True)
    if failed:
        results["stopped_at"] = failed
        print("stopped:", failed, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:                                     # one step per line
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(results[k], sort_keys=True)}" for k in sorted(results)) + "\n}\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
