#!/usr/bin/env python3
"""bench.py — log-marginal-likelihood throughput of the gsum GP hot path on MI355X.

One "step" = one FULL-RECOMPUTE evaluation, the work of one
``TruncationGP.log_marginal_likelihood(theta, ratio=...)`` call in the reference
(gsum/models.py:958-1039, 1485-1507): RBF kernel-matrix build, jittered Cholesky, forward solve,
Gram / log-det reduction, host scalar algebra.  Workload (BASELINE.json configs[2], SURVEY.md §8d "S3"):
n = 8192 1-D points at dx = 0.5 ell, RBF(ell ~ 0.2), nugget 1e-10, 6 EFT orders, synthetic
coefficients; X and the right-hand sides are resident in HBM before the timed region.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

N > 1: one process per GPU; every rank evaluates its own K grid points (weak scaling, no data-path
collective) and the fp64 likelihood slices are all-gathered over RCCL inside the timed region.
Rank 0 prints ONE JSON line.  `python bench.py --gpus N` on its own starts the N ranks itself (child processes of
torch.distributed.run, before this process touches a GPU) and relays rank 0's line.

A plain run sets up, warms up, times ONE region of K steps (bracketed by barrier + synchronize as the contract asks),
writes the outputs of that region if `--dump-outputs DIR` is given (DIR/<name>.npy, float64) and prints the line.
Everything else is behind `--full`: there the timed K-step region is run `--repeats` times back to back (default 10);
`value` / `ms_per_step` are those of the MEDIAN region, min and max are reported beside it.
Beyond the contract's keys a `--full` line carries (N = 1 only, outside the timed regions): `parity` (the GPU value at
ell = 0.2 against the CPU baseline's value of the same evaluation AND against the reference's own committed value,
tests/golden/large_lml.json -- the latter at every N; the run exits non-zero above 1e-10),
`cpu_baseline`, `kernel_time_shares` (HIP-event time of every kernel class inside the timed region), the
single-evaluation stage times, `factor_reuse` (BASELINE config 4's 64 x 64 (cbar, ratio) grid through the product
API), `ell_ratio_grid` (the reference-faithful 64 x 64 (ell, ratio) scan, full recompute) and `predict` (BASELINE
config 5's predictive-variance path, one GPU's share of the new points).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6     # MI355X fp64 matrix peak (AMD spec; vector fp64 is the same rate)
HBM_PEAK_GBS = 8000.0
PARITY_BOUND = 1e-10        # BASELINE.json north_star: log-likelihoods within 1e-10 relative of the scipy path


def make_workload(n, r, seed=0):
    import gsum_amd
    X = 0.1 * np.arange(n)[:, None]
    c = np.random.RandomState(seed).randn(n, r)
    y = gsum_amd.partials(c, ratio=0.5, ref=1.0, orders=np.arange(r))
    return X, y


def available_cpus():
    """CPUs this process may really use: affinity mask and cgroup quota, not the host's core count."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except Exception:
        pass
    return max(1, n)


def host_exp_is_svml():
    """numpy's float64 exp on AVX-512 hosts is Intel SVML's __svml_exp8_ha, which is not correctly rounded (exp(-0.125) comes out one
    ulp low); the device kernel-build restates THAT routine (csrc/kernels/build.hip.h, gs_exp_np) because the reference's own numbers were
    made with it.  On a host whose numpy falls back to libm the CPU leg of this bench would differ from the GPU by ~6e-10 on the
    uniform-grid workload through no fault of either: detected here (behaviour, not CPU flags) and the CPU comparison is then
    labelled instead of failing the run; the committed reference value is the pin at every N either way."""
    import math
    xs = -0.125 * np.arange(0, 75) ** 2.0           # the S2 / S3 kernel arguments
    return bool(np.any(np.exp(xs) != np.array([math.exp(v) for v in xs])) and np.exp(np.full(16, -0.125))[0] == float.fromhex("0x1.c3d6a24ed8221p-1"))


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cpu_baseline(n, r, evals):
    """The CPU oracle (same numpy/scipy/sklearn calls as the reference) on this host's cores, BLAS threads
    = the CPUs this process is allowed to use; plus numpy.linalg.cholesky alone on the same matrix (GF/s)."""
    from sklearn.gaussian_process.kernels import RBF
    from oracle import gsum_oracle as orc
    threads = available_cpus()
    X, y = make_workload(n, r)
    t = []
    val = None
    blas = []
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
        limiter = threadpool_limits(limits=threads)
        blas = [dict(api=i.get("user_api"), lib=i.get("internal_api"), version=i.get("version"),
                     threads=i.get("num_threads"), arch=i.get("architecture")) for i in threadpool_info()]
    except Exception:
        limiter = None
    for i in range(evals):
        t0 = time.perf_counter()
        val = orc.trunc_lml(RBF(0.2), np.log([0.2]), X, y, np.arange(r), ratio=0.5, ref=1.0)
        t.append(time.perf_counter() - t0)
    K = RBF(0.2)(X)
    K[np.diag_indices_from(K)] += 1e-10
    tc = []
    for i in range(2):
        t0 = time.perf_counter()
        np.linalg.cholesky(K)
        tc.append(time.perf_counter() - t0)
    del K
    if limiter is not None:
        limiter.restore_original_limits()
    best = min(t)
    # The BLAS these numbers come from picks its kernels by CPU name: OpenBLAS 0.3.2x does not know Zen 5 and runs its
    # SkylakeX (AVX-512) kernels on an EPYC 9575F.  The same Cholesky under OPENBLAS_CORETYPE=ZEN (AVX2 kernels), in a
    # child process because the library reads the variable when it loads, is recorded beside it.
    alt = None
    try:
        import subprocess
        code = ("import time, numpy as np\nfrom sklearn.gaussian_process.kernels import RBF\n"
                f"X = 0.1 * np.arange({n})[:, None]\nK = RBF(0.2)(X)\nK[np.diag_indices_from(K)] += 1e-10\n"
                "ts = []\nfor i in range(2):\n    t0 = time.perf_counter(); np.linalg.cholesky(K); ts.append(time.perf_counter() - t0)\n"
                "print(min(ts))")
        env = dict(os.environ, OPENBLAS_CORETYPE="ZEN", OPENBLAS_NUM_THREADS=str(threads), OMP_NUM_THREADS=str(threads))
        res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=180)
        alt_s = float(res.stdout.strip().splitlines()[-1])
        alt = dict(coretype="ZEN", cholesky_alone_s=alt_s, cholesky_alone_gflops=n ** 3 / 3.0 / alt_s / 1e9)
    except Exception as exc:
        alt = dict(coretype="ZEN", error=repr(exc))
    return dict(value=1.0 / best, unit="evals/s", cores=int(threads), kind="port",
                blas_note="numpy / scipy ship OpenBLAS built for older cores: on this host it selects by CPU name and runs SkylakeX "
                          "kernels on Zen 5 (see `blas`); a vendor BLAS would be several times faster, so the GPU / CPU ratio says "
                          "little -- the roofline fraction is the figure of merit.  `blas_alt`: the Cholesky alone under "
                          "OPENBLAS_CORETYPE=ZEN.",
                blas_alt=alt,
                sample=f"{evals} full evaluations of oracle.trunc_lml at n={n}, {r} orders (best of {evals}: {best:.2f} s "
                       f"each; all: {', '.join('%.2f' % v for v in t)} s)",
                lml=float(val), cpu_model=cpu_model(), os_cpu_count=os.cpu_count(), blas=blas,
                cholesky_alone_gflops=n ** 3 / 3.0 / min(tc) / 1e9, cholesky_alone_s=min(tc))


def launch_command(n_gpus, port, argv):
    """The command `python bench.py --gpus N` runs when no launcher started it: the contract's own
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...`.
    Pure host logic (tests/test_host_logic.py checks it without a GPU)."""
    # (torch.distributed.run's argparse abbreviates: a bare `--n` among the script's own arguments is "ambiguous" to it)
    argv = ["--points" if a == "--n" else ("--points=" + a[4:] if a.startswith("--n=") else a) for a in argv]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks as children of torch.distributed.run -- before
    this process has touched a GPU, and never by replacing it -- relay their output, return their exit code."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = launch_command(args.gpus, port, sys.argv[1:])
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def golden_lml(n, r):
    """The reference's own value of TruncationGP.log_marginal_likelihood(log 0.2, ratio = 0.5) on make_workload(n, r)
    (tests/golden/large_lml.json, written in the build container by make_golden.py from /root/reference), or None."""
    try:
        with open(os.path.join(ROOT, "tests", "golden", "large_lml.json")) as f:
            for case in json.load(f):
                if case["n"] == n and case["r"] == r and case["seed"] == 0 and case["length_scale"] == 0.2:
                    return float(case["lml"]["0.5"])
    except Exception:
        pass
    return None


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """`--dump-outputs DIR`: every array a caller of the timed path receives as DIR/<name>.npy in float64.  Above 64 MB in all, each
    array keeps a fixed, seeded sample of its leading axis (the same rows on every run of the same arguments) and DIR/<name>_rows.npy
    lists them."""
    os.makedirs(path, exist_ok=True)
    arrays = {name: np.asarray(a, dtype=np.float64) for name, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    for name, a in sorted(arrays.items()):
        if total > DUMP_LIMIT_BYTES and a.ndim > 0 and len(a) > 1:
            keep = max(1, int(len(a) * (DUMP_LIMIT_BYTES // 2) / total))
            rows = np.sort(np.random.RandomState(0).choice(len(a), keep, replace=False))
            np.save(os.path.join(path, f"{name}_rows.npy"), rows.astype(np.float64))
            a = a[rows]
        np.save(os.path.join(path, f"{name}.npy"), a)


def gradient_leg(ctx, X, Z, n):
    """value + analytic gradient pieces of one evaluation (what every L-BFGS step of `fit` costs: gsum_lml_grad)
    and of eight kernels in one call (the restarts of a multi-start fit advance in lock step: gsum_lml_grad_batch), same inputs as the
    headline workload; C * RBF + fixed WhiteKernel, two free hyperparameters."""
    import gsum_amd
    from gsum_amd.kernels import describe_gradient, describe_kernel
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C
    base = C(1.0) * RBF(0.2) + WhiteKernel(1e-10, noise_level_bounds="fixed")
    kernels = [base.clone_with_theta(base.theta + 0.01 * i) for i in range(8)]
    descs, prms = [describe_kernel(k, 1) for k in kernels], [describe_gradient(k, 1) for k in kernels]
    ctx.lml_grad(descs[0], prms[0], X, Z, 1e-10)
    single = []
    for _ in range(3):
        t0 = time.perf_counter()
        one = ctx.lml_grad(descs[0], prms[0], X, Z, 1e-10)
        single.append(time.perf_counter() - t0)
    ctx.lml_grad_batch(descs, prms, X, Z, 1e-10)
    batch = []
    for _ in range(3):
        t0 = time.perf_counter()
        many = ctx.lml_grad_batch(descs, prms, X, Z, 1e-10)
        batch.append(time.perf_counter() - t0)
    same = bool(np.array_equal(many[0][0], one[0]) and np.array_equal(many[4][0], one[4]) and np.array_equal(many[3][0], one[3]))
    flops = float(n) ** 3                    # n^3 / 3 each for the factorisation, U = L^-T and R^-1 = U U^T
    return {"workload": f"value + gradient pieces, n = {n}, 2 free hyperparameters (C * RBF + fixed White)",
            "single_ms": min(single) * 1e3, "batch_of_8_ms_each": min(batch) * 1e3 / 8,
            "single_tflops": flops / min(single) / 1e12, "batch_tflops": 8 * flops / min(batch) / 1e12,
            "flops": "n^3 per evaluation (factorisation, U = L^-T, R^-1 = U U^T: n^3 / 3 each); host wall time, uploads included",
            "batch_equals_single_bit_for_bit": same}


def n2048_leg(ctx):
    """BASELINE configs[1]: n = 2048 1-D RBF, 4 orders -- K build + Cholesky + logpdf on one MI355X.
    One evaluation alone (the multi-kernel path with the persistent chain) and 1024 evaluations of a 512 x 2 (ell, ratio)
    scan through TruncationGP.log_marginal_likelihood_grid(mode="full") (one workgroup per evaluation, k_lml_medium)."""
    import gsum_amd
    from sklearn.gaussian_process.kernels import RBF
    n, r = 2048, 4
    X, y = make_workload(n, r)
    gp = gsum_amd.TruncationGP(kernel=RBF(0.2), ratio=0.5, ref=1.0, center=0, disp=0, df=1, scale=1, optimizer=None)
    gp.fit(X, y, orders=np.arange(r))
    got = float(gp.log_marginal_likelihood(theta=np.log([0.2]), ratio=0.5))
    ts, stage = [], None
    for _ in range(5):
        t0 = time.perf_counter()
        gp.log_marginal_likelihood(theta=np.log([0.2]), ratio=0.5)
        ts.append(time.perf_counter() - t0)
        tm = ctx.timers()
        cur = np.array([tm["build_ms"], tm["potrf_ms"], tm["finalize_ms"], tm["total_ms"]])
        stage = cur if stage is None else np.minimum(stage, cur)
    # 512 length scales x 2 ratios: a ratio row shares its right-hand sides and goes out as one batch of 512 evaluations =
    # one launch of the fused path with every CU holding two evaluations
    ells, ratios = np.linspace(0.15, 0.25, 512), np.linspace(0.45, 0.55, 2)
    thetas = [np.log([e]) for e in ells]
    gp.log_marginal_likelihood_grid(thetas, list(ratios[:1]), mode="full")        # workspaces
    t0 = time.perf_counter()
    grid = gp.log_marginal_likelihood_grid(thetas, list(ratios), mode="full")
    dt = time.perf_counter() - t0
    flops = n ** 3 / 3.0
    ref = golden_lml(n, r)
    # the same 1024 evaluations at the C ABI (gsum_set_inputs + gsum_lml_resident with the descriptors marshalled once): what the
    # device path delivers without the grid method's host work (right-hand sides per ratio row, descriptors, the O(k^2) algebra)
    c = gsum_amd.coefficients(y, 0.5, 1.0, np.arange(r))
    ctx.set_inputs(X, np.concatenate([c, np.ones((n, 1))], axis=1))
    darr = ctx.desc_array([gsum_amd.describe_kernel(RBF(float(e)), 1) for e in np.linspace(0.15, 0.25, 1024)])
    ctx.lml_resident(darr, 1e-10)
    t0 = time.perf_counter()
    _, _, info_abi = ctx.lml_resident(darr, 1e-10)
    dt_abi = time.perf_counter() - t0
    out = {"workload": f"n={n} 1-D RBF(0.2) dx=0.5ell, nugget 1e-10, {r} orders (BASELINE configs[1], S2)",
           "single_eval": {"host_ms_best": min(ts) * 1e3, "gpu_stage_ms": {"kernel_build": stage[0], "cholesky_fused_solve": stage[1],
                                                                          "finalize_d2h": stage[2], "gpu_total": stage[3]},
                           "cholesky_tflops": flops / (stage[1] * 1e-3) / 1e12,
                           "cholesky_frac_of_fp64_mfma_peak": flops / (stage[1] * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                           "note": "one evaluation alone is latency-bound: 8 outer steps of the dependent chain"},
           "grid_1024": {"what": "512 x 2 (ell in linspace(0.15, 0.25), ratio in {0.45, 0.55}) full-recompute scan, "
                                 "log_marginal_likelihood_grid(mode='full'): one workgroup per evaluation (k_lml_medium)",
                         "seconds": dt, "evals_per_s": grid.size / dt, "cholesky_tflops": flops * grid.size / dt / 1e12,
                         "cholesky_frac_of_fp64_mfma_peak": flops * grid.size / dt / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                         "n_neg_inf": int(np.isneginf(grid).sum())},
           "c_abi_1024": {"what": "1024 evaluations (ell in linspace(0.15, 0.25)) through gsum_lml_resident, descriptors marshalled once",
                          "seconds": dt_abi, "evals_per_s": 1024 / dt_abi, "cholesky_tflops": flops * 1024 / dt_abi / 1e12,
                          "cholesky_frac_of_fp64_mfma_peak": flops * 1024 / dt_abi / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                          "n_failed": int(np.count_nonzero(info_abi))},
           "parity": {"gpu": got, "reference": ref, "rel": None if ref is None else abs(got - ref) / abs(ref), "bound": PARITY_BOUND,
                      "what": "TruncationGP.log_marginal_likelihood(log 0.2, ratio=0.5) vs the reference's value, "
                              "tests/golden/large_lml.json (n = 2048)"}}
    return out


def notebook_leg():
    """The reference's own workload (docs/notebooks/correlated_EFT_publication.ipynb:1444-1459: 5 training points, an 80 x 100
    (ratio, ell) surface = 8000 full evaluations) with its flattened kernel RBF + White and with a Sum tree RBF + RBF + White: both run
    one workgroup per evaluation (k_lml_small<false> / <true>); inputs from tests/golden/notebook_grid.json."""
    import gsum_amd
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel
    try:
        with open(os.path.join(ROOT, "tests", "golden", "notebook_grid.json")) as f:
            g = json.load(f)
    except Exception as exc:
        return {"error": repr(exc)}
    X, y = np.array(g["X_train"]), np.array(g["y_train"])
    out = {"workload": "notebook grid: n = 5, 80 ratios x 100 length scales, mode='full' (8000 evaluations per call)"}
    for name, kern in (("flat_rbf_white", RBF(0.2) + WhiteKernel(g["nugget"], noise_level_bounds="fixed")),
                       ("tree_rbf_rbf_white", RBF(0.2) + RBF(2.5, length_scale_bounds="fixed") + WhiteKernel(g["nugget"], noise_level_bounds="fixed"))):
        gp = gsum_amd.TruncationGP(kernel=kern, ref=g["ref"], ratio=0.5, center=0, disp=0, df=1, scale=1, optimizer=None)
        gp.fit(X, y, orders=np.array(g["orders"]))
        thetas = [[t] for t in np.log(g["ls_vals"])]
        gp.log_marginal_likelihood_grid(thetas, g["ratio_vals"], mode="full")
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            grid = gp.log_marginal_likelihood_grid(thetas, g["ratio_vals"], mode="full")
            ts.append(time.perf_counter() - t0)
        rec = {"ms": min(ts) * 1e3, "evals_per_s": grid.size / min(ts), "argmax": [int(v) for v in np.unravel_index(np.argmax(grid), grid.shape)]}
        if name == "flat_rbf_white":
            rec["max_rel_vs_reference_grid"] = float(np.max(np.abs(grid - np.array(g["grid"])) / np.abs(np.array(g["grid"]))))
        out[name] = rec
    out["tree_over_flat"] = out["tree_rbf_rbf_white"]["ms"] / out["flat_rbf_white"]["ms"]
    # fit() with the default optimiser at the notebook's own training-set sizes (models.py:630-669): L-BFGS over objective evaluations with
    # gradient, each ONE launch of k_grad_small; the same class on the cpu backend (numpy / scipy / scikit-learn) beside it
    from sklearn.gaussian_process.kernels import ConstantKernel as C
    fits = {}
    for nn in (5, 20, 64):
        Xf = np.linspace(0, 1, nn)[:, None] * (0.1 * nn + 1.0)
        kern = C(1.0) * RBF(0.5) + WhiteKernel(1e-6, noise_level_bounds="fixed")
        yf = gsum_amd.sample_mvn_cholesky(kern, Xf, 4, nugget=1e-8, random_state=1)
        rec = {}
        for backend in ("hip", "cpu"):
            gpf = gsum_amd.ConjugateGaussianProcess(kernel=kern, center=0, disp=0, df=1, scale=1, backend=backend)
            gpf.fit(Xf, yf)
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                gpf.fit(Xf, yf)
                ts.append(time.perf_counter() - t0)
            th = gpf.kernel_.theta + 0.05
            gpf.log_marginal_likelihood(th, eval_gradient=True)
            t0 = time.perf_counter()
            for _ in range(50):
                gpf.log_marginal_likelihood(th, eval_gradient=True)
            rec[backend] = {"fit_ms": min(ts) * 1e3, "objective_with_gradient_us": (time.perf_counter() - t0) / 50 * 1e6,
                            "length_scale": float(gpf.kernel_.k1.k2.length_scale)}
        fits[f"n{nn}"] = rec
    out["small_fit"] = {"what": "ConjugateGaussianProcess(C * RBF + fixed White).fit with fmin_l_bfgs_b, 4 curves: wall time of fit() and of one "
                                "log_marginal_likelihood(theta, eval_gradient=True); 'cpu' = the same class on numpy / scipy / scikit-learn",
                        **fits}
    return out


def predict_leg(ctx, n, m, reps=3):
    """BASELINE config 5: n 2-D points, Matern-5/2(ell = [0.7, 1.3]) + White(1e-6), 8 curves,
    predictive mean + standard deviation at m new points (2048 = one GPU's share of 16384).  The dominant work is the
    triangular solve V = L^-1 K(X, X*) (n^2 m flops on the matrix cores)."""
    import gsum_amd
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    r = 8
    # box sized so that the mean nearest-neighbour spacing is ~0.5 ell: density 1 / (0.5 ell)^2 per unit area
    side = np.array([0.35, 0.65]) * np.sqrt(n)
    X = np.random.RandomState(0).rand(n, 2) * side
    Xs = np.random.RandomState(1).rand(m, 2) * side
    y = np.random.RandomState(2).randn(n, r)
    kern = Matern(length_scale=[0.7, 1.3], nu=2.5) + WhiteKernel(1e-6, noise_level_bounds="fixed")
    gp = gsum_amd.ConjugateGaussianProcess(kernel=kern, center=0, disp=0, df=1, scale=1, optimizer=None)
    fit_all, fit_diag = [], []
    for _ in range(3):                       # (the first fit of a process also allocates the 2.2-GB workspace: all are reported)
        t0 = time.perf_counter()
        gp.fit(X, y)
        fit_all.append(time.perf_counter() - t0)
        fit_diag.append({"chain_aborts": ctx.get_option("chain_aborts"), "chain_persist": ctx.get_option("chain_persist"),
                         "potrf_ms": ctx.timers()["potrf_ms"]})
    fit_s = min(fit_all)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        mean, std = gp.predict(Xs, return_std=True)
        ts.append(time.perf_counter() - t0)
    best = min(ts)
    parity = None
    try:
        # BASELINE config 5 as specified: the reference's own fit / predict at the first 16 of these new points
        # (tests/golden/s5_predict.json, generated in the build container; same recipe as above)
        with open(os.path.join(ROOT, "tests", "golden", "s5_predict.json")) as f:
            g5 = json.load(f)
        if g5["n"] == n and g5["m"] == m and g5["r"] == r:
            p16 = g5["probes"]
            wm, wv = np.array(g5["mean"]), np.array(g5["std"]) ** 2
            lml = float(gp.log_marginal_likelihood(theta=np.log([0.7, 1.3])))
            parity = {"what": "HIP fit + predict(return_std) at the first 16 new points and log_marginal_likelihood vs the reference's "
                              "own outputs on the same S5 inputs (tests/golden/s5_predict.json; models.py:753-845)",
                      "mean_max_abs_over_max_mean": float(np.max(np.abs(mean[:p16] - wm)) / np.max(np.abs(wm))),
                      "var_max_abs_over_cov_factor": float(np.max(np.abs(std[:p16] ** 2 - wv)) / g5["cov_factor"]),
                      "cov_factor_rel": abs(float(gp.cov_factor_) - g5["cov_factor"]) / g5["cov_factor"],
                      "lml_rel": abs(lml - g5["lml"]) / abs(g5["lml"]),
                      "bounds": {"mean": 1e-9, "var": 1e-10, "cov_factor": 1e-10, "lml": PARITY_BOUND}}
            parity["rel"] = max(parity["var_max_abs_over_cov_factor"], parity["lml_rel"], parity["cov_factor_rel"])
            parity["ok"] = bool(parity["mean_max_abs_over_max_mean"] <= 1e-9 and parity["var_max_abs_over_cov_factor"] <= 1e-10
                                and parity["cov_factor_rel"] <= 1e-10 and parity["lml_rel"] <= PARITY_BOUND)
    except Exception as exc:
        parity = {"error": repr(exc), "ok": False}
    flops = float(n) * n * m            # TRSM on the new points' columns: n^2 m
    return {"workload": f"n={n} 2-D Matern-5/2(ell=[0.7,1.3]) + White(1e-6), {r} curves, m={m} new points "
                        f"(BASELINE configs[4], S5; m = one GPU's share of 16384)",
            "fit_ms": fit_s * 1e3, "fit_ms_all": [v * 1e3 for v in fit_all], "fit_schedule": fit_diag, "predict_ms": best * 1e3, "predict_ms_all": [v * 1e3 for v in ts],
            "points_per_s": m / best,
            "roofline": {"kernel": "triangular solve of the new points' columns on the bulk MFMA tile", "bound": "mfma",
                         "achieved": flops / best / 1e12, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": flops / best / 1e12 / FP64_MFMA_PEAK_TFLOPS, "flops": "n^2 m",
                         "note": "end to end (host wall time of predict(), uploads and read-back included)"},
            "parity": parity,
            "finite": bool(np.isfinite(mean).all() and np.isfinite(std).all()), "std_mean": float(np.mean(std))}


def inproc_main(args):
    """`bench.py --inproc N`: the contract's workload and JSON keys with the N GPUs driven from ONE process through the C ABI's device
    group (include/gsum_hip.h: gsum_init_multi, gsum_group_set_inputs, gsum_group_lml_resident) -- what a single-process caller of the
    reference (docs/notebooks/correlated_EFT_publication.ipynb:1444-1459) gets from `log_marginal_likelihood_grid(devices=...)`.  Weak
    scaling like --gpus N: every device evaluates its own K grid points (block partition, gsum_shard_range), the gather of the grid
    (--gather rccl: one in-place ncclAllGather over the devices) is inside the timed region."""
    import torch
    import gsum_amd
    from sklearn.gaussian_process.kernels import RBF
    from gsum_amd.conjugate import lml_from_gram_batch

    n, r, K, W, N = args.n, args.orders, args.steps, args.warmup, args.inproc
    ids = [int(v) for v in args.devices.split(",")] if args.devices else list(range(N))
    if len(ids) != N:
        raise SystemExit(f"--inproc {N} but --devices lists {len(ids)}")
    repeated = len(set(ids)) != len(ids)
    gather = "host" if repeated else args.gather              # RCCL wants one rank per GPU
    grp = gsum_amd.HipGroup(ids, own=True) if repeated else gsum_amd.default_group(ids)
    ctx0 = grp.contexts[0]
    X, y = make_workload(n, r)
    c = gsum_amd.coefficients(y, 0.5, 1.0, np.arange(r))
    Z = np.concatenate([c, np.ones((n, 1))], axis=1)
    jac = float(np.sum(np.arange(r)) * np.log(0.5) * n)
    grp.set_inputs(X, Z)                                      # X, RHS resident in the HBM of every device from here on
    if args.groups > 0:
        grp.set_option("wave_groups", args.groups)
    if args.group_size > 0:
        grp.set_option("wave_size", args.group_size)
    total = N * K
    ells = np.linspace(0.19, 0.21, total) if total > 1 else np.array([0.2])
    descs = ctx0.desc_array([gsum_amd.describe_kernel(RBF(float(e)), 1) for e in ells])

    last = {}

    def evaluate(batch, how):
        G, sld, info = grp.lml_resident(batch, 1e-10, gather=how)
        out = lml_from_gram_batch(G, sld, n, 0.0, 0.0, 1, 1) - jac
        out[np.asarray(info) != 0] = -np.inf
        last.update(gram=G, sum_log_diag=sld, info=info)
        return out

    def sync_all():
        for d in set(ids):
            torch.cuda.synchronize(d)

    evaluate(descs, gather)                                   # set-up: workspaces on every device, the communicators
    for _ in range(max(0, -(-W // max(1, K)))):
        evaluate(descs, gather)

    def timed_region(profile_every=0):
        ctx0.set_option("profile_gemm", profile_every)
        ctx0.kernel_profile()
        sync_all()
        t0 = time.perf_counter()
        vals = evaluate(descs, gather)
        sync_all()
        el = time.perf_counter() - t0
        return el, vals, ctx0.kernel_profile()

    regions = [timed_region() for _ in range(max(1, args.repeats))]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, dict(last, lml=regions[-1][1]))
    order = sorted(range(len(regions)), key=lambda i: regions[i][0])
    elapsed, allvals, _ = regions[order[(len(order) - 1) // 2]]
    all_elapsed = [reg[0] for reg in regions]
    groups, gsize = ctx0.get_option("wave_groups"), ctx0.get_option("wave_size")
    out = {"metric": "lml_evals_per_sec", "value": total / elapsed, "unit": "evals/s", "n_gpus": N, "steps": K, "warmup": W,
           "ms_per_step": elapsed / K * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
           "data": "synthetic",
           "config": {"workload": f"full-recompute lml eval: n={n} 1-D RBF(ell~0.2) dx=0.5ell, nugget 1e-10, {r} orders"
                                  + (" (BASELINE configs[2], S3)" if (n, r) == (8192, 6) else " (not the headline size: rehearsal)"),
                      "n": n, "orders": r, "evals_per_gpu": K, "mode": "full-recompute",
                      "parallelism": f"inproc{N}: ONE process, the library's device group -- one gsum_ctx and one host thread per GPU "
                                     f"(devices {ids}), descriptors block-partitioned (gsum_shard_range), gather = {gather}"
                                     + (" (a device is listed twice: contexts of their own, RCCL not applicable)" if repeated else ""),
                      "batch_schedule": f"{groups} groups x up to {min(gsize, -(-K // groups))} evaluations per device and call; "
                                        f"{ctx0.get_option('wave_streams')} streams per device"},
           "repeats": {"n": len(all_elapsed), "stat": "median region (lower median)", "ms_per_step_median": elapsed / K * 1e3,
                       "ms_per_step_min": min(all_elapsed) / K * 1e3, "ms_per_step_max": max(all_elapsed) / K * 1e3,
                       "evals_per_s_all": [total / e for e in all_elapsed]},
           "gathered": {"length": int(len(allvals)), "expected": int(total), "finite": bool(np.isfinite(allvals).all())},
           "lml_sample": float(allvals[0])}
    if not args.full:
        print(json.dumps(out), flush=True)
        return 0 if np.isfinite(allvals).all() else 3
    prof_elapsed, _, prof = timed_region(1)
    ctx0.set_option("profile_gemm", 0)
    gemm_ms, gemm_flops, gemm_launches = (prof["bulk_update"][k] for k in ("ms", "flops", "launches"))
    launch_tflops = gemm_flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
    # every device's first grid point again, as a single evaluation on device 0 (another schedule, another GPU): bit-identical or rc 3
    firsts = [int(gsum_amd.shard_range(total, rk, N)[0]) for rk in range(N)]
    G1, s1, i1 = zip(*[ctx0.lml_resident([descs[i]], 1e-10) for i in firsts])
    redo = lml_from_gram_batch(np.concatenate(G1), np.concatenate(s1), n, 0.0, 0.0, 1, 1) - jac
    got_first = np.array([allvals[i] for i in firsts])
    rank_check = {"what": "grid point 0 of every device's block: gathered value vs a single evaluation of the same descriptor on the "
                          "first device", "ranks": N, "bit_identical": bool(np.array_equal(redo, got_first)),
                  "max_rel": float(np.max(np.abs(redo - got_first) / np.abs(redo)))}
    gpu_lml_02 = float(lml_from_gram_batch(*ctx0.lml_resident([gsum_amd.describe_kernel(RBF(0.2), 1)], 1e-10)[:2], n, 0.0, 0.0, 1, 1)[0] - jac)
    ref_v = golden_lml(n, r)
    ref_rel = None if ref_v is None else abs(gpu_lml_02 - ref_v) / abs(ref_v)
    out.update({
        "roofline": {"kernel": "k_gemm_ld3g on the first device of the group (every device runs the same launches)", "bound": "mfma",
                     "achieved": launch_tflops, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": launch_tflops / FP64_MFMA_PEAK_TFLOPS, "traffic": None, "launches": gemm_launches,
                     "avg_launch_us": gemm_ms * 1e3 / max(1, gemm_launches), "sum_launch_ms": gemm_ms, "region_ms": elapsed * 1e3,
                     "busy_share_of_region": gemm_ms * 1e-3 / prof_elapsed},
        "group": {"devices": ids, "rccl": grp.get("rccl"), "rccl_gathers": grp.get("rccl_gathers"),
                  "devices_used": grp.get("devices_used"), "pipes_ok": [c_.get_option("pipes_ok") for c_ in grp.contexts]},
        "rank_check": rank_check,
        "parity": {"gpu": gpu_lml_02, "reference": ref_v, "rel": ref_rel, "bound": PARITY_BOUND,
                   "status": "checked" if ref_rel is not None else "unchecked: no committed reference value for this size",
                   "what": "TruncationGP.log_marginal_likelihood(log 0.2, ratio=0.5) on the first device vs the reference's committed "
                           "value (tests/golden/large_lml.json)"}})
    print(json.dumps(out), flush=True)
    rc = 0
    if (ref_rel is not None and not ref_rel <= PARITY_BOUND) or not rank_check["bit_identical"] or not np.isfinite(allvals).all():
        rc = 3
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20,
                    help="evaluations per timed region = per call of the batch entry point (default: one round of the library's "
                         "3 groups, 7 + 7 + 6 evaluations)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", "--points", dest="n", type=int, default=8192)
    ap.add_argument("--orders", type=int, default=6)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: repeated regions, per-kernel profile and roofline, parity against the reference and "
                         "the CPU baseline, the other configurations (grids, predict, n = 2048, notebook, gradient)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed region computed as DIR/<name>.npy (float64)")
    ap.add_argument("--cpu-evals", type=int, default=3, help="--full: CPU-baseline evaluations (0 = skip)")
    ap.add_argument("--repeats", type=int, default=None,
                    help="the timed K-step region is run this many times back to back; value / ms_per_step are the "
                         "median region, min and max are reported beside it (default: 1, with --full 10)")
    ap.add_argument("--groups", type=int, default=0, help="groups of the batch schedule (0 = library default, 3)")
    ap.add_argument("--group-size", type=int, default=0, help="evaluations per group at most (0 = library default, 8)")
    ap.add_argument("--inproc", type=int, default=0,
                    help="N > 0: the same weak-scaling workload over N GPUs from THIS process -- the library's device group "
                         "(gsum_init_multi / gsum_group_lml_resident: one context and one host thread per GPU inside the library), "
                         "no torch.distributed; prints the same JSON keys as --gpus N")
    ap.add_argument("--devices", default="", help="--inproc: comma-separated device indices (default 0 .. N-1; an index may repeat "
                                                  "to rehearse the fan-out on one GPU: contexts of their own then)")
    ap.add_argument("--gather", default="rccl", choices=["host", "rccl"],
                    help="--inproc: how the grid comes together -- host: every device's thread writes its block into the caller's "
                         "arrays; rccl (default): additionally one in-place ncclAllGather between the devices inside the timed region")
    ap.add_argument("--backend", default="nccl", help="process-group backend for N > 1 (nccl = RCCL; gloo to rehearse)")
    ap.add_argument("--device", type=int, default=None, help="GPU index override (rehearsal: several ranks on one GPU)")
    ap.add_argument("--config", default="lml", choices=["lml", "predict"],
                    help="lml: the headline line; predict: only BASELINE config 5's predictive-variance leg (for profiling)")
    ap.add_argument("--extras", type=int, default=1, help="--full, 0: skip the legs outside the contract (grids, predict)")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 10 if args.full else 1

    if args.inproc > 0:
        raise SystemExit(inproc_main(args))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args))

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dev = local_rank if args.device is None else args.device
    use_dist = "WORLD_SIZE" in os.environ            # launched by torch.distributed.run (also with one rank)
    if use_dist:
        torch.cuda.set_device(dev)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
        else:
            dist.init_process_group(args.backend)
    if use_dist and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import gsum_amd
    from sklearn.gaussian_process.kernels import RBF
    from gsum_amd.conjugate import lml_from_gram_batch
    from gsum_amd.grid import gather_flat

    n, r, K, W = args.n, args.orders, args.steps, args.warmup
    ctx = gsum_amd.default_context(dev)
    if args.config == "predict":
        out = predict_leg(ctx, 16384, 2048, reps=8)
        if rank == 0:
            print(json.dumps({"metric": "predict_points_per_sec", "value": out["points_per_s"], "unit": "points/s",
                              "n_gpus": 1, "higher_is_better": True, "dtype": "f64", "data": "synthetic",
                              "config": {"workload": out["workload"]}, "predict": out}), flush=True)
        return
    X, y = make_workload(n, r)
    c = gsum_amd.coefficients(y, 0.5, 1.0, np.arange(r))
    Z = np.concatenate([c, np.ones((n, 1))], axis=1)
    jac = float(np.sum(r * np.log(np.abs(np.ones(n))) + np.sum(np.arange(r)) * np.log(np.abs(0.5 * np.ones(n)))))
    ctx.set_inputs(X, Z)                     # X, RHS resident in HBM from here on

    # this rank's grid points: length scales around 0.2 (every point is a distinct evaluation)
    total = world * K
    ells = np.linspace(0.19, 0.21, total) if total > 1 else np.array([0.2])
    mine = ells[rank * K:(rank + 1) * K]
    descs = [gsum_amd.describe_kernel(RBF(float(e)), 1) for e in mine]

    last = {}

    def evaluate(batch):
        """K build + Cholesky + fused solve for every descriptor (one call of the batch entry point: the library advances them in
        groups, one launch per kernel class and outer step), then the O(k^2) host algebra per evaluation."""
        G, sld, info = ctx.lml_resident(batch, 1e-10)
        out = lml_from_gram_batch(G, sld, n, 0.0, 0.0, 1, 1) - jac          # the O(k^2) algebra of all evaluations in one numpy pass
        out[np.asarray(info) != 0] = -np.inf
        last.update(gram=G, sum_log_diag=sld, info=info)
        return out

    if args.groups > 0:
        ctx.set_option("wave_groups", args.groups)
    if args.group_size > 0:
        ctx.set_option("wave_size", args.group_size)
    # set-up, not a step: the groups' workspaces (0.55 GB per evaluation in flight) are allocated on first use; do that here so
    # that a small --warmup does not leave hipMalloc calls inside the timed region.  A call of 4 x groups x size evaluations or more
    # (the library's threshold for a second cohort per group) allocates every workspace a longer call uses, so the set-up call is no
    # longer than that.  It is repeated for one second: the first of ten back-to-back regions ran ~0.4 % below their median while the
    # clocks settled, and a plain run times one region.
    groups, gsize = ctx.get_option("wave_groups"), ctx.get_option("wave_size")
    setup = [descs[i % len(descs)] for i in range(max(3, min(K, 4 * groups * gsize)))]
    t_setup = time.perf_counter()
    evaluate(setup)
    while time.perf_counter() - t_setup < 1.0:
        evaluate(setup)
    in_flight = min(K, groups * gsize)
    gsize = min(gsize, -(-K // groups))            # a call shorter than groups x size fills the groups equally
    if W > 0:
        evaluate([descs[i % len(descs)] for i in range(W)])
    if use_dist:
        gather_flat(np.zeros(K), total)          # warm-up of the collective (RCCL sets its rings up lazily)
    def timed_region(profile_every=0):
        ctx.set_option("profile_gemm", profile_every)
        ctx.kernel_profile()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vals = evaluate(descs)
        allv = gather_flat(vals, total) if use_dist else vals       # one all-gather of the fp64 slices (RCCL)
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        el = time.perf_counter() - t0
        if use_dist:
            tt = torch.tensor([el], dtype=torch.float64, device="cuda" if args.backend == "nccl" else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            el = float(tt.item())
        prof = ctx.kernel_profile()
        return el, allv, prof

    # `repeats` plain timed regions (value = their median), then, with --full, ONE more region with HIP events around every launch
    # (a batch is ~170 launches since round 4: bracketing them all costs ~1 %): per-kernel times inside a timed region, each on the
    # stream it is launched on.  The profiled region is reported, not counted.
    regions = [timed_region() for _ in range(max(1, args.repeats))]
    if rank == 0 and args.dump_outputs:          # what the last timed region computed (N > 1: lml is the gathered grid)
        dump_outputs(args.dump_outputs, dict(last, lml=regions[-1][1]))
    order = sorted(range(len(regions)), key=lambda i: regions[i][0])
    elapsed, allvals, _ = regions[order[(len(order) - 1) // 2]]        # the median region (lower median)
    all_elapsed = [reg[0] for reg in regions]
    head = {
        "metric": "lml_evals_per_sec", "value": total / elapsed, "unit": "evals/s",
        "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": elapsed / K * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": f"full-recompute lml eval: n={n} 1-D RBF(ell~0.2) dx=0.5ell, nugget 1e-10, {r} orders"
                               + (" (BASELINE configs[2], S3)" if (n, r) == (8192, 6) else
                                  " (BASELINE configs[1], S2)" if (n, r) == (2048, 4) else " (not a BASELINE size: rehearsal)"),
                   "n": n, "orders": r,
                   "evals_per_gpu": K, "mode": "full-recompute", "evals_in_flight_per_gpu": in_flight,
                   "batch_schedule": ("fewer than three evaluations per call: one after the other on the single-factorisation schedule "
                                      "(persistent chain); " if K < 3 else
                                      f"{groups} groups x up to {gsize} evaluations, one launch per kernel class and outer step; ")
                                     + f"{ctx.get_option('wave_streams')} streams; GPU_MAX_HW_QUEUES "
                                     + ("unset" if "GPU_MAX_HW_QUEUES" not in os.environ else os.environ["GPU_MAX_HW_QUEUES"])},
        "repeats": {"n": len(all_elapsed), "stat": "median region (lower median)",
                    "ms_per_step_median": elapsed / K * 1e3, "ms_per_step_min": min(all_elapsed) / K * 1e3,
                    "ms_per_step_max": max(all_elapsed) / K * 1e3,
                    "evals_per_s_all": [total / e for e in all_elapsed]},
    }
    if not args.full:                            # the plain run: the headline and nothing that takes runs of its own
        finite = bool(np.isfinite(allvals).all())
        if rank == 0:
            print(json.dumps(dict(head, lml_sample=float(allvals[0]),
                                  gathered={"length": int(len(allvals)), "expected": int(total), "finite": finite})), flush=True)
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        if len(allvals) != total or not finite:
            raise SystemExit(3)
        return
    prof_elapsed, _, prof = timed_region(1)
    ctx.set_option("profile_gemm", 0)
    gemm_ms, gemm_flops, gemm_launches = (prof["bulk_update"][k] for k in ("ms", "flops", "launches"))

    # every rank's first grid point, recomputed on rank 0 as a single evaluation (a different schedule: one factorisation alone):
    # the gathered value must be that number bit for bit -- same code object, same inputs (N > 1: a rank that gathered garbage or
    # another rank's slice fails here; N = 1: the batch against the single evaluation)
    rank_check = None
    if rank == 0:
        firsts = [float(ells[rk * K]) for rk in range(world)]
        redo = np.array([evaluate([gsum_amd.describe_kernel(RBF(e), 1)])[0] for e in firsts])
        got_first = np.array([allvals[rk * K] for rk in range(world)])
        rank_check = {"what": "grid point 0 of every rank: gathered value vs a single evaluation of the same descriptor on rank 0",
                      "ranks": int(world), "bit_identical": bool(np.array_equal(redo, got_first)),
                      "max_rel": float(np.max(np.abs(redo - got_first) / np.abs(redo)))}

    # single-evaluation stage times (one evaluation alone on the GPU), outside the timed region
    stage = None
    for i in range(3):
        ctx.lml_resident([descs[0]], 1e-10)
        tm = ctx.timers()
        cur = np.array([tm["build_ms"], tm["potrf_ms"], tm["finalize_ms"], tm["total_ms"]])
        stage = cur if stage is None else np.minimum(stage, cur)
    single_schedule = {"chain_probe": ctx.get_option("chain_probe"), "chain_aborts": ctx.get_option("chain_aborts"),
                       "chain_persist": ctx.get_option("chain_persist"),
                       "what": "schedule of ONE factorisation alone: chain_probe 1 = persistent chain kernel in use, -1 = this process' "
                               "streams do not run side by side (e.g. under a serialising profiler): host-enqueued look-ahead schedule; "
                               "chain_aborts > 0: a chain timed out and the evaluation was re-run on the host-enqueued schedule"}
    ctx.set_option("profile_gemm", 1)
    ctx.kernel_profile()
    ctx.lml_resident([descs[0]], 1e-10)
    single_prof = ctx.kernel_profile()
    ctx.set_option("profile_gemm", 0)
    # parity inside the run: the evaluation the CPU baseline times (ell = 0.2 exactly), on the GPU
    gpu_lml_02 = float(evaluate([gsum_amd.describe_kernel(RBF(0.2), 1)])[0])

    # dominant kernel, exclusive: one SYRK launch of the step-0 shape alone on the GPU (device-resident random
    # operands), for the kernel-quality view next to the in-situ numbers
    # (200 back-to-back launches, 60 ms: the sustained rate.  A handful of launches after an idle gap read 20 % low
    # while the clock ramps; under this kernel the package sits at its 1400 W cap with sclk ~2.34 GHz,
    # profiles/r02_clock_power.log -- the 78.6 TFLOP/s peak assumes 2.4 GHz.)
    # (the microbenchmark entry point is not part of the product ABI: it lives in the lab build of the library, include/gsum_hip_debug.h)
    excl_tflops = excl_k256 = None
    try:
        lab = gsum_amd.lab_context(dev)
        lab.bench_gemm_nt(7, n - 256, n - 256, 256, True, n + 16, 20)
        excl_k256, _ = lab.bench_gemm_nt(7, n - 256, n - 256, 256, True, n + 16, 200)
        if n > 2048:                         # the shape the batch launches: four panels deep (K = 1024), the trailing matrix of outer step 3
            lab.bench_gemm_nt(7, n - 1024, n - 1024, 1024, True, n + 16, 5)
            excl_tflops, _ = lab.bench_gemm_nt(7, n - 1024, n - 1024, 1024, True, n + 16, 50)
        else:
            excl_tflops = excl_k256
        lab.set_option("release_scratch", 1)
    except Exception as exc:                 # no lab library on this box: the in-situ per-launch figure stands alone
        print(f"[bench] exclusive microbenchmark skipped: {exc}", file=sys.stderr)

    reuse = ell_grid = pred = cfg2 = grad = nb = by_order = None
    if rank == 0 and world == 1 and args.extras:
        cfg2 = n2048_leg(ctx)
        nb = notebook_leg()
        grad = gradient_leg(ctx, X, Z, n)
        ctx.set_inputs(X, Z)                 # (the leg above used the operator-level inputs; the resident set is untouched, but be explicit)
        orders = np.arange(r)
        gp = gsum_amd.TruncationGP(kernel=RBF(0.2), ratio=0.5, ref=1.0, center=0, disp=0, df=1, scale=1, optimizer=None)
        gp.X_train_, gp.y_train_, gp.orders_ = X, y, orders
        # factor-reuse mode, reported separately and never mixed into `value`: BASELINE config 4's
        # 64 x 64 (cbar, ratio) grid at ONE kernel costs one K build + Cholesky + forward solve; ratio rescales the Gram
        # matrix order by order, the prior scale (cbar = sd) only enters the O(k^2) host algebra
        cbars, ratios = np.geomspace(0.25, 4, 64), np.linspace(0.3, 0.7, 64)
        t1 = time.perf_counter()
        grid = gp.log_marginal_likelihood_grid([np.log([0.2])], list(ratios), scales=cbars, mode="reuse")[:, 0, :]
        dt = time.perf_counter() - t1
        reuse = {"grid": "64 x 64 (ratio in linspace(0.3, 0.7), cbar = sd prior in geomspace(0.25, 4)) at one kernel, "
                         "TruncationGP.log_marginal_likelihood_grid(scales=..., mode='reuse')",
                 "seconds": dt, "evals_per_s": grid.size / dt, "mode": "factor-reuse",
                 "argmax": [int(v) for v in np.unravel_index(np.argmax(grid), grid.shape)],
                 "n_neg_inf": int(np.isneginf(grid).sum()),
                 "note": "white-noise coefficients (timing workload): the maximum sits on the cbar boundary; index parity on "
                         "GP-drawn data is tests/test_gpu_config4.py"}
        # the reference-faithful scan (notebook :1444-1459): 64 length scales x 64 ratios, every point recomputed
        ell_axis = np.linspace(0.05, 0.5, 64)
        # set-up, not part of the scan: a call of 96 evaluations or more runs two cohorts per group and allocates the second cohort's
        # workspaces (13 GB) on first use
        gp.log_marginal_likelihood_grid([np.log([e]) for e in ell_axis], list(ratios[:2]), mode="full")
        t1 = time.perf_counter()
        g2 = gp.log_marginal_likelihood_grid([np.log([e]) for e in ell_axis], list(ratios), mode="full")
        dt = time.perf_counter() - t1
        ell_grid = {"grid": "64 x 64 (ratio in linspace(0.3, 0.7), ell in linspace(0.05, 0.5)), mode='full': 4096 evaluations, "
                            "each its own K build + Cholesky + solve; since round 5 the 64 rows' right-hand sides are resident as 64 sets and "
                            "the surface is ONE call (gsum_lml_resident_sets): 171 rounds of the groups back to back",
                    "seconds": dt, "evals_per_s": g2.size / dt, "n_neg_inf": int(np.isneginf(g2).sum()),
                    "argmax": [int(v) for v in np.unravel_index(np.argmax(g2), g2.shape)], "mode": "full-recompute"}
        ctx.set_option("release_scratch", 1)
        pred = predict_leg(ctx, 16384, 2048, reps=5)
        ctx.set_option("release_scratch", 1)
        # ONE factorisation alone against the order (the stage timer of a single evaluation: kernel build and solve excluded): the dependent
        # chain of a 256-column step costs ~116 us whatever the order, so the fraction of the fp64 peak grows with n
        by_order = {}
        for nn in (2048, 4096, 8192, 16384, 32768):
            Xn = 0.1 * np.arange(nn)[:, None]
            Zn = np.concatenate([np.random.RandomState(0).randn(nn, r), np.ones((nn, 1))], axis=1)
            ctx.set_inputs(Xn, Zn)
            dn = gsum_amd.describe_kernel(RBF(0.2), 1)
            best = None
            for _ in range(3):
                _, _, info_n = ctx.lml_resident([dn], 1e-10)
                ms = ctx.timers()["potrf_ms"]
                best = ms if best is None else min(best, ms)
            by_order[str(nn)] = {"potrf_ms": best, "tflops": nn ** 3 / 3.0 / (best * 1e-3) / 1e12,
                                 "frac_of_fp64_mfma_peak": nn ** 3 / 3.0 / (best * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS, "info": int(info_n[0])}
            ctx.set_option("release_scratch", 1)
        ctx.set_inputs(X, Z)

    pmc_traffic = pmc_file = pmc_alg = None
    pmc_what = ""
    for name in ("r05_gemm_pmc.json", "r04_gemm_pmc.json", "r03_gemm_pmc.json", "r02_gemm_pmc.json", "r01_gemm_pmc.json"):          # the newest committed counter passes
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                rec = json.load(f)
            pmc_traffic = rec["derived"]["hbm_traffic_bytes_per_launch"]
            pmc_alg = rec["derived"].get("algorithmic_bytes_per_launch")
            pmc_what = rec.get("what", "HBM bytes of one M=8192, K=256 launch of this kernel's tile (FETCH_SIZE x 2 KiB + WRITE_SIZE x 1 KiB)")
            pmc_file = name
            break
        except Exception:
            pass
    rc = 0
    if rank == 0:
        potrf_flops = n ** 3 / 3.0
        chol_tflops = potrf_flops / (stage[1] * 1e-3) / 1e12
        # all ranks run the same launches; rank 0's record stands for one GPU
        launch_tflops = gemm_flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0    # algorithmic flops of the bulk launches / the sum
                                                                                    # of their durations (they do not overlap one another)
        region_tflops = gemm_flops / elapsed / 1e12                                   # ... / wall time of the median timed region
        bytes_written = 4.0 * n * n + 4.0 * n * 128
        shares = {name: {"ms_per_eval": v["ms"] / K, "launches_per_region": v["launches"],
                         "share_of_region_time": v["ms"] * 1e-3 / prof_elapsed}
                  for name, v in prof.items()}
        out = {
            **head,
            "single_eval_stage_ms": {"kernel_build": stage[0], "cholesky_fused_solve": stage[1],
                                     "finalize_d2h": stage[2], "gpu_total": stage[3]},
            "single_eval_schedule": single_schedule,
            "single_eval_kernel_ms": {name: {"ms": v["ms"], "launches": v["launches"]} for name, v in single_prof.items()},
            "cholesky": {"single_eval_gflops": chol_tflops * 1e3,
                         "single_eval_frac_of_fp64_mfma_peak": chol_tflops / FP64_MFMA_PEAK_TFLOPS,
                         "pipelined_gflops_per_gpu": potrf_flops * K / elapsed / 1e9,
                         "pipelined_frac_of_fp64_mfma_peak": potrf_flops * K / elapsed / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                         "flops": "n^3/3", "single_eval_ms": stage[1],
                         "single_eval_by_order": by_order if rank == 0 and world == 1 and args.extras else None},
            "kernel_build": {"gbps_bytes_written": bytes_written / (stage[0] * 1e-3) / 1e9,
                             "frac_of_hbm_peak": bytes_written / (stage[0] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                             "bytes_written": "lower-triangle tiles only (4n^2 + 4n*128): what the kernel stores",
                             "us": stage[0] * 1e3},
            # dominant kernel: the fp64-MFMA SYRK of the trailing update, k_gemm_ld3g.  Since round 4 a launch carries one outer step
            # of all members of a group and the groups' launches follow one another on ONE stream: `achieved` is the prescribed
            # per-launch figure -- algorithmic flops of the launches / the sum of their HIP-event durations on that stream -- and
            # it is what `rocprofv3 --kernel-trace --stats` of this command reports for the kernel (profiles/).
            "roofline": {"kernel": "k_gemm_ld3g (128x64-tile, 8-wave fp64 MFMA SYRK with LDS-direct operand staging, 3 workgroups "
                                   "per CU; one launch = the trailing update of every evaluation of a group, four panels deep: K = 1024 (512 / 256 near the end))",
                         "bound": "mfma", "achieved": launch_tflops, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": launch_tflops / FP64_MFMA_PEAK_TFLOPS, "traffic": pmc_traffic,
                         "traffic_source": f"{pmc_what}; from the committed rocprofv3 --pmc passes, profiles/{pmc_file} (PMC cannot be "
                                           "collected inside bench.py)",
                         "algorithmic_bytes_per_launch": pmc_alg,
                         "traffic_over_algorithmic": (pmc_traffic / pmc_alg) if pmc_traffic and pmc_alg else None,
                         "launches": gemm_launches,
                         "launches_sampled": "every launch of one extra, profiled K-step region "
                                             f"({prof_elapsed / K * 1e3:.3f} ms per step with the events in place)",
                         "avg_launch_us": gemm_ms * 1e3 / max(1, gemm_launches),
                         "avg_flops_per_launch": gemm_flops / max(1, gemm_launches),
                         "sum_launch_ms": gemm_ms, "region_ms": elapsed * 1e3,
                         "busy_share_of_region": gemm_ms * 1e-3 / prof_elapsed,
                         "region_tflops": region_tflops, "region_frac": region_tflops / FP64_MFMA_PEAK_TFLOPS,
                         "exclusive_tflops": excl_tflops,
                         "exclusive_frac": None if excl_tflops is None else excl_tflops / FP64_MFMA_PEAK_TFLOPS,
                         "exclusive_what": "the same tile alone on the chip (lab microbenchmark, device-resident random operands): 50 back-to-back "
                                           "lower-triangle launches of the batch's far-update shape at outer step 3 (M = n - 1024, K = 1024)",
                         "exclusive_tflops_K256": excl_k256,
                         "exclusive_K256_what": "... and of the one-product shape rounds 1-3 reported (M = n - 256, K = 256: 200 launches)",
                         "flops_per_launch": "algorithmic flops of each launch: lower-triangular SYRK M(M+1)K per member (K = 256 x the panels "
                                             "it applies); the near updates (the next panel's 256 columns, K <= 768) run on the chain "
                                             "streams (k_gemm_ld3n) and are counted with the panel class"},
            "kernel_time_shares": {"classes": shares,
                                   "note": "HIP-event duration of every launch inside one extra timed K-step region (not counted in "
                                           "value), per kernel class, on the launch's own stream; share = class time / that region's "
                                           "wall time.  The bulk class runs on one stream (its share is the fraction of the region "
                                           "the trailing updates occupy the chip); diagonal blocks, panels and kernel builds run on "
                                           "the groups' chain streams BESIDE it, so the shares add up to more than 1",
                                   "profiled_region_ms_per_step": prof_elapsed / K * 1e3,
                                   "sum_of_shares": float(sum(v["share_of_region_time"] for v in shares.values()))},
            "rank_check": rank_check,
            "streams": {"pipes_ok": ctx.get_option("pipes_ok"), "pipe_overlap_permille": ctx.get_option("pipe_overlap_permille"),
                        "streams_replaced_at_init": ctx.get_option("pipe_heals"),
                        "what": "gsum_init's pairwise probe of the context's four streams (100-us kernels): 1 = every pair ran side by side"},
            "factor_reuse": reuse,
            "ell_ratio_grid": ell_grid,
            "predict": pred,
            "n2048": cfg2,
            "notebook_grid": nb,
            "gradient": grad,
            "lml_sample": float(allvals[0]),
        }
        ref_v = golden_lml(n, r)
        ref_rel = None if ref_v is None else abs(gpu_lml_02 - ref_v) / abs(ref_v)
        ref_what = ("the reference's own value of the same evaluation, tests/golden/large_lml.json (written in the build "
                    "container from /root/reference): checked at every N")
        if world == 1 and args.cpu_evals > 0:
            out["cpu_baseline"] = cpu_baseline(n, r, args.cpu_evals)
            out["speedup_vs_cpu"] = out["value"] / out["cpu_baseline"]["value"]
            cpu_v = out["cpu_baseline"]["lml"]
            rel = abs(gpu_lml_02 - cpu_v) / abs(cpu_v)
            out["parity"] = {"gpu": gpu_lml_02, "cpu": cpu_v, "rel": rel, "bound": PARITY_BOUND, "reference": ref_v,
                             "rel_vs_reference": ref_rel, "reference_what": ref_what,
                             "what": "TruncationGP.log_marginal_likelihood(log 0.2, ratio=0.5) of the S3 workload: HIP path vs the "
                                     "CPU oracle evaluation that cpu_baseline times"}
            svml = host_exp_is_svml()
            out["parity"]["host_exp_is_svml"] = svml
            if not svml:
                out["parity"]["cpu_note"] = ("this host's numpy exp is NOT the SVML routine the reference's numbers were made with and the "
                                             "device kernel build restates: the CPU leg's kernel matrix differs by an ulp on whole diagonals "
                                             "(~6e-10 on the log-likelihood); the CPU comparison is reported, the pin is rel_vs_reference")
            elif not rel <= PARITY_BOUND:
                rc = 3
        else:
            out["parity"] = {"gpu": gpu_lml_02, "cpu": None, "rel": ref_rel, "bound": PARITY_BOUND, "reference": ref_v,
                             "rel_vs_reference": ref_rel, "reference_what": ref_what,
                             "what": "TruncationGP.log_marginal_likelihood(log 0.2, ratio=0.5) of the workload on rank 0's GPU vs the "
                                     "reference's committed value (no CPU leg at N > 1 / --cpu-evals 0)"}
        # never exit 0 with no numeric gate having run and nothing said about it
        cpu_checked = out["parity"].get("cpu") is not None and out["parity"].get("host_exp_is_svml", False)
        out["parity"]["status"] = ("checked" if (ref_rel is not None or cpu_checked) else
                                   "unchecked: no committed reference value for this size and no CPU leg that can be compared "
                                   "(--cpu-evals 0, N > 1, or a host whose numpy exp is not SVML)")
        if out["parity"]["status"] != "checked":
            print("[bench] parity UNCHECKED: " + out["parity"]["status"], file=sys.stderr)
        if ref_rel is not None and not ref_rel <= PARITY_BOUND:
            rc = 3
        if pred is not None and pred.get("parity") is not None and not pred["parity"].get("ok", False):
            rc = 3
        if cfg2 is not None and cfg2["parity"]["rel"] is not None and not cfg2["parity"]["rel"] <= PARITY_BOUND:
            rc = 3
        # N > 1: every rank's slice came through the all-gather; the gathered grid must be complete and finite
        out["gathered"] = {"length": int(len(allvals)), "expected": int(total), "finite": bool(np.isfinite(allvals).all())}
        if len(allvals) != total or not np.isfinite(allvals).all():
            rc = 3
        if rank_check is not None and not rank_check["bit_identical"]:
            rc = 3
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rc:
        raise SystemExit(rc)


if __name__ == "__main__":
    main()
