"""The blocked route of the Toeplitz path on one device.  Writes one JSON file.

    python tools/gpu_toeplitz_blocked.py [--out profiles/toeplitz_blocked_<date>.json] [--timeout 300] [--only TEXT]

Part 1, where all three routes exist: ``toeplitz_predict`` at n = 8192 with q = 256 and 2048 new points (no covariance) and
``toeplitz_gram`` on the 64 x 64 (length scale, ratio) surface of section 18 at n = 2048 and 8192 (64 first columns, 64 sets of 6
columns), each through ``method="columns"``, ``"panel"`` and ``"blocked"``: wall time and the device milliseconds by phase.

Part 2, beyond the other routes' limit: one ARFIMA(0, 0.4, 0) first column with five right-hand sides through
``toeplitz_gram(method="blocked")`` at n = 16384, 65536, 262144 and 1048576: wall and phase times, ``sum_log_diag`` against the closed
form in units of 2^-53, and the device memory the handle holds after the call (the device's free memory before the handle opens minus
after the call, and the library's own arithmetic beside it).  The dense route's recorded single factorisation at n = 16384 stands beside
the first.

Whether ``uniform_grid_step`` accepts ``numpy.linspace(0, 1, 2**20)`` is recorded too (no device).

Every step runs in a child process of its own under its own time limit (``--step NAME`` is what the child runs); the first step that
fails or runs out of time ends the run, and what was measured until then is still written.  Wall times are host arrays to host result,
one warm-up and then two calls: the best and the spread of the two; the device milliseconds by phase are those of the last call."""
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

METHODS = ("columns", "panel", "blocked")
NEW_POINTS = (256, 2048)
SURFACE_SIZES = (2048, 8192)
SURFACE = dict(m=64, n_sets=64, cols=6)
LARGE = (16384, 65536, 262144, 1048576)
DENSE_POTRF_MS_AT_16384 = 26.9                       # the dense route's single factorisation, as recorded in DESIGN.md


def steps():
    out = [f"predict:{method}:8192:{q}" for q in NEW_POINTS for method in METHODS]
    out += [f"surface:{method}:{n}" for n in SURFACE_SIZES for method in METHODS]
    return out + [f"large:blocked:{n}" for n in LARGE]


def arfima_column(n, d):
    t = [1.0]
    for k in range(1, n):
        t.append(t[-1] * (k - 1 + d) / (k - d))
    return np.array(t)


def arfima_sum_log_diag(n, d):
    """sum_j log L_jj = 1/2 sum_k (n - k) log1p(-gamma_k^2), gamma_k = d / (k - d), in long double."""
    ld = np.longdouble
    k = np.arange(1, n, dtype=ld)
    g = ld(d) / (k - ld(d))
    return float(np.sum((n - k) * np.log1p(-g * g)) / 2)


def timed_twice(call):
    call()
    walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    return dict(wall_s=min(walls), wall_spread_s=abs(walls[0] - walls[1]))


def reset(h):
    for clock in (h.times, h.post_times, h.panel_times, h.blocked_times):
        clock(reset=True)


def clocks(h, method, column_clock):
    ms = {"panel": h.panel_times, "blocked": h.blocked_times}.get(method, column_clock)()
    out = dict(device_ms_by_phase=ms, device_ms=sum(ms.values()))
    if method == "panel":
        out["recursion_ms"] = ms["recursion"]
    if method == "blocked":
        out["recursion_ms"] = ms["lead"] + ms["tiles"]
    return out


def predict(h, method, n, q):
    import gsum_amd as gm
    rng = np.random.RandomState(0)
    t, K, Z = arfima_column(n, 0.4), rng.randn(n, q), rng.randn(n, 3)

    def call():
        reset(h)
        assert gm.toeplitz_predict(t, K, Z, method=method).info == 0

    out = dict(method=method, n=n, q=q, **timed_twice(call))
    out.update(clocks(h, method, h.post_times))
    return out


def surface(h, method, n):
    import gsum_amd as gm
    m, n_sets, cols = (SURFACE[k] for k in ("m", "n_sets", "cols"))
    t = np.stack([arfima_column(n, 0.4 - 0.005 * i) for i in range(m)])
    Z = np.random.RandomState(0).randn(n, n_sets * cols)

    def call():
        reset(h)
        assert not gm.toeplitz_gram(t, Z, n_sets, method=method)[2].any()

    out = dict(method=method, n=n, **SURFACE, **timed_twice(call))
    out.update(clocks(h, method, h.times))
    return out


def large(n, free_before):
    import torch
    import gsum_amd as gm
    from gsum_amd import _toep_lib
    h = _toep_lib.default_handle(0)
    d, c = 0.4, 5
    t, Z = arfima_column(n, d), np.random.RandomState(0).randn(n, c)
    got = {}

    def call():
        reset(h)
        got["G"], got["sld"], got["info"] = gm.toeplitz_gram(t, Z, 1, method="blocked")
        assert got["info"] == 0

    out = dict(method="blocked", n=n, cols=c, d=d, **timed_twice(call))
    out.update(clocks(h, "blocked", None))
    truth = arfima_sum_log_diag(n, d)
    B, R = gm.toeplitz_panel_width(), _toep_lib.blocked_tile_rows()
    out.update(sum_log_diag=got["sld"], closed_form=truth, sum_log_diag_error_eps=abs(got["sld"] - truth) / max(1.0, abs(truth)) / 2.0 ** -53,
               G_finite=bool(np.isfinite(got["G"]).all()), panel_width=B, tile_rows=R, lead_us_per_step=1e3 * out["device_ms_by_phase"]["lead"] / n,
               device_bytes_held=int(free_before - torch.cuda.mem_get_info(0)[0]),
               device_bytes_by_the_library_s_arithmetic=int(n * c * 12 + n * B * 12 + (9 * n + 4 * B) * 8))
    if n == 16384:
        out["dense_potrf_ms_recorded"] = DENSE_POTRF_MS_AT_16384
    return out


def grid_check():
    import gsum_amd as gm
    try:
        return dict(accepted=True, step=gm.uniform_grid_step(np.linspace(0, 1, 2 ** 20)[:, None]))
    except ValueError as e:
        return dict(accepted=False, error=str(e))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", f"toeplitz_blocked_{datetime.date.today().isoformat()}.json"))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--only", default=None, help="run the steps that contain this text")
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    if args.step:
        kind, method, *rest = args.step.split(":")
        if kind == "large":
            import torch
            res = large(int(rest[0]), torch.cuda.mem_get_info(0)[0])
        else:
            from gsum_amd import _toep_lib
            h = _toep_lib.default_handle(0)
            res = predict(h, method, int(rest[0]), int(rest[1])) if kind == "predict" else surface(h, method, int(rest[0]))
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    results, failed = {"uniform_grid_step:linspace_2^20": grid_check()}, None
    for step in [s for s in steps() if args.only is None or args.only in s]:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            failed = f"{step}: no result within {args.timeout} s"
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            failed = f"{step}: exit status {p.returncode}: {p.stderr[-2000:]}"
            break
        results[step] = json.loads(lines[-1][7:])
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
