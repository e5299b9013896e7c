#!/usr/bin/env python3
"""Generate tests/golden/variogram.json from the reference's own VariogramFourthRoot and Diagnostic.variogram.

Runs ONLY where a checkout of the reference (buqeye/gsum) is available; the file it writes holds data only -- seeded inputs and the
reference's outputs.  Usage:  GSUM_REFERENCE=<checkout of buqeye/gsum> python tests/golden/make_golden_variogram.py

``import gsum`` needs docrep, seaborn and statsmodels' MVT, absent here: they are in-memory placeholder modules as in
make_golden_diagnostics.py.  No numeric code is stubbed.
"""
import base64
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GSUM_REFERENCE", os.path.join(HERE, "..", "..", "..", "reference"))


def _import_reference():
    d = types.ModuleType("docrep")

    class _DP:
        def __init__(self, *a, **k):
            pass

        def get_sectionsf(self, *a, **k):
            return lambda f: f

        def dedent(self, f):
            return f

    d.DocstringProcessor = _DP
    sys.modules["docrep"] = d
    sys.modules["seaborn"] = types.ModuleType("seaborn")
    for name in ("statsmodels", "statsmodels.sandbox", "statsmodels.sandbox.distributions",
                 "statsmodels.sandbox.distributions.mv_normal"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["statsmodels.sandbox.distributions.mv_normal"].MVT = object
    sys.path.insert(0, REF)
    import gsum  # noqa
    from gsum import diagnostics, helpers  # noqa
    return diagnostics, helpers


diagnostics, helpers = _import_reference()
from sklearn.gaussian_process.kernels import RBF  # noqa: E402


def L(a):
    """float64 bytes (little-endian, base64) and shape; tests decode with np.frombuffer(base64.b64decode(v["f64"]), "<f8")"""
    a = np.array(a, dtype="<f8", order="C")
    return {"f64": base64.b64encode(a.tobytes()).decode(), "shape": list(a.shape)}


def rule_bounds(X):
    """GraphicalDiagnostic.variogram's bins (diagnostics.py:589-590), nbins as an int (current numpy rejects the float)"""
    N = len(X)
    nbins = np.ceil((N * (N - 1) / 2.) ** (1. / 3))
    return np.linspace(0, np.max(np.linalg.norm(X, axis=-1)), int(nbins))


def gp_curves(X, n, rng, ls=0.3):
    K = RBF(ls)(X) + 1e-8 * np.eye(len(X))
    return (np.linalg.cholesky(K) @ rng.standard_normal((len(X), n))).T


def inputs(rng):
    out = []
    X = np.sort(rng.uniform(0, 1, 60))[:, None]
    out.append(("a_d1_gp3", X, gp_curves(X, 3, rng), rule_bounds(X)))
    X = rng.uniform(0, 1, (40, 2))
    out.append(("b_d2_1d_z", X, gp_curves(X, 1, rng)[0], rule_bounds(X)))
    X = (np.arange(30) * 0.1 + rng.uniform(0, 0.02, 30))[:, None]          # every distance >= 0.08: bin 0 empty, gamma~[0] NaN
    out.append(("c_empty_bin0", X, gp_curves(X, 2, rng, 0.8), np.linspace(0.05, 3.0, 12)))
    X = rng.uniform(0, 1, (35, 1))
    out.append(("d_pairs_below_bound0", X, gp_curves(X, 2, rng), np.linspace(0.1, 0.9, 8)))
    g = np.arange(6.0)
    X = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)          # distances 1, 2, 3, ... land on the bounds
    out.append(("e_integer_grid", X, gp_curves(X, 2, rng, 2.0), np.arange(1.0, 8.0)))
    X = np.sort(rng.uniform(0, 1, 30))[:, None]
    X[5:10] = X[0:5]                                                           # duplicate points: h = 0
    out.append(("f_duplicates", X, rng.standard_normal((2, 30)), rule_bounds(X)))
    X = np.sort(rng.uniform(0, 1, 30))[:, None]
    z = np.vstack([gp_curves(X, 1, rng), np.full((1, 30), 1.5)])               # a constant curve: gamma~ = 0
    out.append(("g_constant_curve", X, z, rule_bounds(X)))
    X = rng.uniform(0, 1, (40, 9))
    out.append(("h_d9", X, rng.standard_normal((2, 40)), rule_bounds(X)))
    return out


def case(name, X, z, bounds, rng):
    v = helpers.VariogramFourthRoot(X, z, bounds)
    Nb, Nc = v.Nb, v.Ncurves
    cov_diag = np.array([np.broadcast_to(v.cov(b), (Nc,)) for b in range(Nb)])
    full = np.flatnonzero(v.bin_counts)
    pairs = [(int(full[0]), int(full[-1])), (int(full[len(full) // 2]), int(full[0])), (int(full[1]), int(full[2]))]
    cov_off = np.array([np.broadcast_to(v.cov(a, b), (Nc,)) for a, b in pairs])
    for c in range(Nc):                             # no stored covariance within rounding of 0 (the NaN pattern of sqrt is stable)
        col = np.concatenate([cov_diag[:, c], cov_off[:, c]])
        fin = col[np.isfinite(col) & (col != 0)]
        if fin.size:
            assert np.min(np.abs(fin)) > 1e-9 * np.max(np.abs(fin)), (name, c)
    rec = dict(name=name, X=L(X), z=L(z), bounds=L(bounds), bin_counts=[int(c) for c in v.bin_counts],
               bin_locations=L(v.bin_locations), gamma_star_hat=L(v.gamma_star_hat), gamma_star_mean=L(v.gamma_star_mean),
               gamma_tilde=L(v.gamma_tilde), cov_diag=L(cov_diag), cov_pairs=pairs, cov_off=L(cov_off))
    for rt in (False, True):
        gam, lo, up = v.compute(rt_scale=rt)
        rec[f"compute_{int(rt)}"] = [L(gam), L(lo), L(up)]
    _, loc, gam, lo, up = diagnostics.Diagnostic.variogram(X, z, bounds)
    rec["diagnostic_variogram"] = [L(loc), L(gam), L(lo), L(up)]
    N = len(X)
    idx = rng.randint(0, N, (4, 12))
    idx[2:, :3] = idx[:2, :3]                       # (i, j) == (k, l) for some
    rec["ijkl"] = idx.tolist()
    rec["rho_ijkl"] = L(v.rho_ijkl(*idx))
    rec["corr_ijkl"] = L(v.corr_ijkl(*idx))
    rec["cov_ijkl"] = L(v.cov_ijkl(*idx))
    rec["var_ij"] = L(v.var_ij(idx[0], idx[1]))
    if name.startswith("b_"):                        # the lazy O(P) attributes of one small case
        rec["inputs_hij"] = L(v.inputs.hij)
        rec["inputs_bin_idxs"] = v.inputs.bin_idxs.tolist()
        rec["bin_idx"] = v.bin_idx.tolist()
        rec["data_dij"] = L(v.data.dij)
        rec["gamma_tilde_grid"] = L(v.gamma_tilde_grid)
    return rec


def main():
    warnings.simplefilter("ignore", RuntimeWarning)
    rng = np.random.RandomState(20261016)
    cases = [case(name, X, z, b, rng) for name, X, z, b in inputs(rng)]
    path = os.path.join(HERE, "variogram.json")
    with open(path, "w") as f:
        json.dump(dict(cases=cases), f)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
