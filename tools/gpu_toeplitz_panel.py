"""The panel route of the Toeplitz path against the column route on one device: ``toeplitz_predict`` at n = 2048 and
8192 with q = 256 and 2048 new points, with and without the covariance (the table of section 20), and ``toeplitz_gram`` on the 64 x 64
(length scale, ratio) surface of section 18 at n = 2048 and 8192 with five curves (64 first columns, 64 sets of 6 columns), each through
``method="columns"`` and ``method="panel"``.  Writes one JSON file.

    python tools/gpu_toeplitz_panel.py [--out profiles/toeplitz_panel_<date>.json] [--timeout 300] [--lib libgsum_toep_variant.so]

Every step runs in a child process of its own under its own time limit (``--step NAME`` is what the child runs); the first step that
fails or runs out of time ends the run, and what was measured until then is still written.  ``--lib`` loads another build of the
library (one compiled with -DGSUM_TOEP_PANEL_B=<width>) in place of the package's.

Inputs: the first columns are ARFIMA(0, d, 0) autocovariances (d = 0.4 for predict, 0.4 - 0.005 i for first column i of the surface),
the columns seeded normals.  Wall times are host arrays to host result, one warm-up and then two calls: the best and the spread of the
two; the device milliseconds by phase are those of the last call.  ``recursion_share`` is the recursion phase over all device time of
the panel route."""
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
METHODS = ("columns", "panel")
SURFACE = dict(m=64, n_sets=64, cols=6)


def steps():
    out = [f"predict:{method}:{n}:{q}:{what}" for n in SIZES for q in NEW_POINTS for what in ("std", "cov") for method in METHODS]
    return out + [f"surface:{method}:{n}" for n in SIZES for method in METHODS]


def arfima_column(n, d):
    t = [1.0]
    for k in range(1, n):
        t.append(t[-1] * (k - 1 + d) / (k - d))
    return np.array(t)


def timed_twice(call):
    call()
    walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    return dict(wall_s=min(walls), wall_spread_s=abs(walls[0] - walls[1]))


def handle(lib):
    from gsum_amd import _toep_lib
    if lib:
        _toep_lib.LIB_PATH = os.path.abspath(lib)
    return _toep_lib.default_handle(0)


def clocks(h, method, column_clock):
    """The device milliseconds of the last call: the panel clock's, or the column route's own (``times`` or ``post_times``)."""
    ms = h.panel_times() if method == "panel" else column_clock()
    out = dict(device_ms_by_phase=ms, device_ms=sum(ms.values()))
    if method == "panel":
        out["recursion_share"] = ms["recursion"] / out["device_ms"]
    return out


def predict(h, method, n, q, what):
    import gsum_amd as gm
    rng = np.random.RandomState(0)
    t, K, Z = arfima_column(n, 0.4), rng.randn(n, q), rng.randn(n, 3)

    def call():
        h.panel_times(reset=True)
        h.post_times(reset=True)
        assert gm.toeplitz_predict(t, K, Z, want_cov=what == "cov", method=method).info == 0

    out = dict(method=method, n=n, q=q, what=what, panel_width=gm.toeplitz_panel_width(), **timed_twice(call))
    out.update(clocks(h, method, h.post_times))
    return out


def surface(h, method, n):
    import gsum_amd as gm
    m, n_sets, cols = (SURFACE[k] for k in ("m", "n_sets", "cols"))
    t = np.stack([arfima_column(n, 0.4 - 0.005 * i) for i in range(m)])
    Z = np.random.RandomState(0).randn(n, n_sets * cols)

    def call():
        h.panel_times(reset=True)
        h.times(reset=True)
        assert not gm.toeplitz_gram(t, Z, n_sets, method=method)[2].any()

    out = dict(method=method, n=n, panel_width=gm.toeplitz_panel_width(), **SURFACE, **timed_twice(call))
    out.update(clocks(h, method, h.times))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", f"toeplitz_panel_{datetime.date.today().isoformat()}.json"))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--only", default=None, help="run the steps that contain this text")
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    if args.step:
        kind, method, *rest = args.step.split(":")
        h = handle(args.lib)
        res = predict(h, method, int(rest[0]), int(rest[1]), rest[2]) if kind == "predict" else surface(h, method, int(rest[0]))
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    results, failed = {}, None
    for step in [s for s in steps() if args.only is None or args.only in s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + (["--lib", args.lib] if args.lib else [])
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
    for step in [s for s in results if ":panel:" in s]:
        other = step.replace(":panel:", ":columns:")
        if other in results:
            a, b = results[step], results[other]
            results[step.replace(":panel:", ":panel_over_columns:")] = dict(
                wall=a["wall_s"] / b["wall_s"], device=a["device_ms"] / b["device_ms"],
                beyond_spread=bool(abs(a["wall_s"] - b["wall_s"]) > a["wall_spread_s"] + b["wall_spread_s"]))
    if failed:
        results["stopped_at"] = failed
        print("stopped:", failed, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:                                     # one step per line
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(results[k], sort_keys=True)}" for k in sorted(results)) + "\n}\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
