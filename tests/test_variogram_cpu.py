"""VariogramFourthRoot / Diagnostic.variogram on backend='cpu' against the reference's fixture (tests/golden/variogram.json), the
argument checks, and the C ABI of libgsum_vario.so (symbol table only: no GPU needed)."""
import base64
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

import gsum_amd as gm
from conftest import ROOT, load_golden


def A(v):
    return np.frombuffer(base64.b64decode(v["f64"]), "<f8").reshape(v["shape"])


def same_nan(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))


def close(got, want, rtol=0, atol=0):
    same_nan(got, want)
    m = ~np.isnan(np.asarray(want, dtype=float))
    np.testing.assert_allclose(np.asarray(got, dtype=float)[m], np.asarray(want, dtype=float)[m], rtol=rtol, atol=atol)


def cov_close(got, want):
    """cov <= 1e-10 x max|cov| of that curve (columns), identical NaN masks"""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    same_nan(got, want)
    for c in range(want.shape[1]):
        col = want[:, c]
        fin = np.isfinite(col)
        if fin.any():
            np.testing.assert_allclose(got[fin, c], col[fin], rtol=0, atol=1e-10 * np.max(np.abs(col[fin])))


def band_close(got, want):
    fin = np.isfinite(want)
    close(got, want, rtol=1e-9, atol=1e-12 * (np.max(np.abs(want[fin])) if fin.any() else 0))


def check_case(case, backend):
    """Every value of one fixture case through ``backend``; returns the object."""
    X, z, bounds = A(case["X"]), A(case["z"]), A(case["bounds"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        v = gm.VariogramFourthRoot(X, z, bounds, backend=backend)
        np.testing.assert_array_equal(v.bin_counts, case["bin_counts"])
        assert v.Nb == len(bounds) + 1 and v.N == len(X) and v.Ncurves == A(case["gamma_tilde"]).shape[1]
        np.testing.assert_array_equal(v.bin_labels, np.arange(v.Nb))
        close(v.bin_locations, A(case["bin_locations"]), rtol=1e-12)
        close(v.gamma_star_hat, A(case["gamma_star_hat"]), rtol=1e-12)
        close(v.gamma_star_mean, A(case["gamma_star_mean"]), rtol=1e-11)
        close(v.gamma_tilde, A(case["gamma_tilde"]), rtol=1e-11)
        cov_diag = np.array([np.broadcast_to(v.cov(b), (v.Ncurves,)) for b in range(v.Nb)])
        cov_close(cov_diag, A(case["cov_diag"]))
        cov_off = np.array([np.broadcast_to(v.cov(a, b), (v.Ncurves,)) for a, b in case["cov_pairs"]])
        cov_close(cov_off, A(case["cov_off"]))
        for rt in (0, 1):
            got = v.compute(rt_scale=bool(rt))
            want = [A(w) for w in case[f"compute_{rt}"]]
            close(got[0], want[0], rtol=1e-11)
            band_close(got[1], want[1])
            band_close(got[2], want[2])
        out = gm.Diagnostic.variogram(X, z, bounds, backend=backend)
        want = [A(w) for w in case["diagnostic_variogram"]]
        assert isinstance(out[0], gm.VariogramFourthRoot)
        close(out[1], want[0], rtol=1e-12)
        close(out[2], want[1], rtol=1e-11)
        band_close(out[3], want[2])
        band_close(out[4], want[3])
        out[0].close()
    return v


@pytest.fixture(scope="module")
def golden():
    return load_golden("variogram.json")["cases"]


def test_cpu_backend_matches_the_reference(golden):
    assert len(golden) == 8
    for case in golden:
        check_case(case, "cpu")


def test_cpu_lazy_attributes_and_host_methods_are_bit_equal(golden):
    for case in golden:
        X, z, bounds = A(case["X"]), A(case["z"]), A(case["bounds"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            v = gm.VariogramFourthRoot(X, z, bounds, backend="cpu")
            np.testing.assert_array_equal(v.gamma_tilde, A(case["gamma_tilde"]))        # the reference's np.average: same bits
            np.testing.assert_array_equal(v.bin_locations, A(case["bin_locations"]))
            i, j, k, l = np.array(case["ijkl"])  # noqa: E741
            np.testing.assert_array_equal(v.rho_ijkl(i, j, k, l), A(case["rho_ijkl"]))
            np.testing.assert_array_equal(v.corr_ijkl(i, j, k, l), A(case["corr_ijkl"]))
            np.testing.assert_array_equal(v.cov_ijkl(i, j, k, l), A(case["cov_ijkl"]))
            np.testing.assert_array_equal(v.var_ij(i, j), A(case["var_ij"]))
            if "inputs_hij" in case:
                np.testing.assert_array_equal(v.inputs.hij, A(case["inputs_hij"]))
                np.testing.assert_array_equal(v.inputs.bin_idxs, case["inputs_bin_idxs"])
                np.testing.assert_array_equal(v.bin_idx, case["bin_idx"])
                np.testing.assert_array_equal(v.data.dij, A(case["data_dij"]))
                np.testing.assert_array_equal(v.gamma_tilde_grid, A(case["gamma_tilde_grid"]))
                np.testing.assert_array_equal(v.bin_mask, v.bin_labels[:, None] == np.array(case["bin_idx"]))
                ti, tj = np.tril_indices(len(X), -1)
                np.testing.assert_array_equal(v.inputs.i, ti)
                np.testing.assert_array_equal(v.inputs.j, tj)


def test_argument_errors():
    X = np.linspace(0, 1, 10)[:, None]
    z = np.sin(X[:, 0])
    b = np.linspace(0, 1, 4)
    with pytest.raises(ValueError, match="z must have shape"):
        gm.VariogramFourthRoot(X, z[:9], b, backend="cpu")
    with pytest.raises(ValueError, match="z must have shape"):
        gm.VariogramFourthRoot(X, np.vstack([z, z]).T, b, backend="cpu")
    with pytest.raises(ValueError, match="non-decreasing"):
        gm.VariogramFourthRoot(X, z, b[::-1], backend="cpu")
    with pytest.raises(ValueError, match="finite"):
        gm.VariogramFourthRoot(X, z, np.array([0, np.inf]), backend="cpu")
    Xn = X.copy()
    Xn[3, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        gm.VariogramFourthRoot(Xn, z, b, backend="cpu")
    with pytest.raises(ValueError, match="features"):
        gm.VariogramFourthRoot(np.zeros((10, 65)), z, b, backend="cpu")
    with pytest.raises(ValueError, match="32767"):
        gm.VariogramFourthRoot(X, z, np.arange(32767.0), backend="cpu")
    with pytest.raises(ValueError, match="non-empty"):
        gm.VariogramFourthRoot(X, z, np.array([]), backend="cpu")
    with pytest.raises(ValueError, match="n_samples"):
        gm.VariogramFourthRoot(X[:, 0], z, b, backend="cpu")
    with pytest.raises(ValueError, match="backend"):
        gm.VariogramFourthRoot(X, z, b, backend="cuda")
    v = gm.VariogramFourthRoot(X, z, b, backend="cpu")
    with pytest.raises(IndexError):
        v.cov(v.Nb)
    np.testing.assert_array_equal(v.cov(-1), v.cov(v.Nb - 1))
    assert "VariogramFourthRoot" in gm.__all__


def test_empty_bins():
    X = np.linspace(0, 1, 12)[:, None]
    z = np.cos(3 * X[:, 0])
    v = gm.VariogramFourthRoot(X, z, np.array([5.0, 6.0]), backend="cpu")     # bins 1 and 2 are empty
    assert v.cov(1) == 0. and v.cov(0, 2) == 0.
    assert np.isnan(v.gamma_star_hat[1:]).all()
    np.testing.assert_array_equal(v.bin_counts, [66, 0, 0])


def test_vario_library_exports_exactly_its_header():
    from gsum_amd import _vario_lib
    from gsum_amd import build as _b
    path = _b.build_vario()
    header = open(os.path.join(ROOT, "include", "gsum_vario.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(gsum_vario_[a-z0-9_]+)\s*\(", body))
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}            # every defined dynamic symbol, unfiltered
    assert exported == declared, exported ^ declared
    assert set(_vario_lib.PROTOTYPES) == declared


def test_coefficient_generator_reproduces_the_header():
    pytest.importorskip("mpmath")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_vario_coeffs.py"), "--check"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
