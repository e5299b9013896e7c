"""gsum_amd.refdist on backend='cpu' against direct numpy, its argument checks, and the export table of libgsum_refdist.so against
include/gsum_refdist.h (the library is cross-compiled for gfx950; no GPU is needed to read its symbols)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import gsum_amd as gm  # noqa: E402
from gsum_amd import refdist  # noqa: E402

SHAPES = [(n, m) for n in (1, 2, 17, 1000) for m in (1, 2, 17, 1000)]
QS = [0.0, 100.0, 2.5, 16.0, 50.0, 84.0, 97.5]


def _inputs(n, m, kind, seed=0):
    rng = np.random.RandomState(seed + 7 * n + m)
    A = rng.standard_normal((n, m))
    r = rng.uniform(size=A.shape)
    if kind == "tied":
        A = np.round(A, 1)
    elif kind == "zeros":
        A[r < 0.3] = 0.0
        A[(r >= 0.3) & (r < 0.6)] = -0.0
    elif kind == "inf":
        A[r < 0.1] = np.inf
        A[(r >= 0.1) & (r < 0.2)] = -np.inf
    elif kind == "nan":
        A[r < 0.1] = np.nan
        A[(r >= 0.1) & (r < 0.15)] = -np.nan
    return A


def _linear_percentile(S, q):
    """numpy's 'linear' method written out on sorted rows (the formula of include/gsum_refdist.h)"""
    m = S.shape[1]
    v = (m - 1) * (np.asarray(q) / 100)
    i = np.minimum(np.floor(v).astype(int), m - 1)
    g = (v - np.floor(v))[:, None]
    a, b = S[:, i].T, S[:, np.minimum(i + 1, m - 1)].T
    with np.errstate(invalid="ignore"):
        out = np.where(g >= 0.5, b - (b - a) * (1 - g), a + (b - a) * g)
    out[:, np.isnan(S[:, -1])] = np.nan
    return out


@pytest.mark.parametrize("kind", ["random", "tied", "zeros", "inf", "nan"])
@pytest.mark.parametrize("n,m", SHAPES)
def test_cpu_backend_is_numpy(n, m, kind):
    A = _inputs(n, m, kind)
    S = np.sort(A, axis=0)
    np.testing.assert_array_equal(refdist.sort_columns(A, backend="cpu"), S)
    with np.errstate(invalid="ignore"):
        want = np.percentile(A, QS, axis=1)
        got = refdist.row_percentiles(A, QS, backend="cpu")
        np.testing.assert_array_equal(got, want)
        bands, srt = refdist.qq_bands(A, QS, return_sorted=True, backend="cpu")
        np.testing.assert_array_equal(srt, S)
        np.testing.assert_array_equal(bands, np.percentile(S, QS, axis=1))
        np.testing.assert_array_equal(refdist.qq_bands(A, QS, backend="cpu"), bands)
        if kind != "inf":                   # (inf - inf is NaN in either form; which form numpy takes there is its own business)
            np.testing.assert_array_equal(got, _linear_percentile(np.sort(A, axis=1), QS))


@pytest.mark.parametrize("K", [1, 3, 101])
@pytest.mark.parametrize("n,m", [(1, 1), (2, 17), (17, 2), (1000, 17)])
def test_cpu_interval_coverage(n, m, K):
    rng = np.random.RandomState(n + m + K)
    Y = rng.standard_normal((n, m))
    half = rng.uniform(0, 2.5, (K, 1)) * rng.uniform(0.5, 1.5, (1, n))
    lower, upper = -half, half.copy()
    lower[0, 0] = Y[0, 0]                                            # on a bound: not inside
    upper[K - 1, n - 1] = Y[n - 1, m - 1]
    Y[n // 2, m // 2] = np.nan
    got = refdist.interval_coverage(Y, lower, upper, backend="cpu")
    counts = np.zeros((m, K), dtype=np.int64)
    for j in range(m):
        for k in range(K):
            counts[j, k] = np.sum((lower[k] < Y[:, j]) & (Y[:, j] < upper[k]))
    assert got.shape == (m, K)
    np.testing.assert_array_equal(got, counts / n)


def test_backend_resolution_and_refusals(monkeypatch):
    A = np.arange(12.0).reshape(4, 3)
    monkeypatch.setenv("GSUM_BACKEND", "cpu")
    np.testing.assert_array_equal(refdist.sort_columns(A[::-1]), A)
    with pytest.raises(ValueError):
        refdist.sort_columns(A, backend="cuda")
    for bad in ([-1.0], [100.5], [np.nan], []):
        with pytest.raises(ValueError):
            refdist.row_percentiles(A, bad)
    with pytest.raises(ValueError):
        refdist.sort_columns(np.zeros(3))
    with pytest.raises(ValueError):
        refdist.sort_columns(np.zeros((0, 3)))
    with pytest.raises(ValueError):
        refdist.interval_coverage(A, np.zeros((2, 3)), np.zeros((2, 3)))        # bounds must be (K, n = 4)
    assert gm.refdist is refdist


def test_refdist_library_exports_every_declared_symbol():
    """include/gsum_refdist.h is the contract of libgsum_refdist.so: every function it declares is exported and bound, nothing else."""
    from gsum_amd import _refdist_lib, build
    header = open(os.path.join(ROOT, "include", "gsum_refdist.h")).read()
    declared = set(re.findall(r"\b(gsum_refdist_[a-z0-9_]+)\s*\(", header))
    assert declared and declared == set(_refdist_lib.PROTOTYPES), declared ^ set(_refdist_lib.PROTOTYPES)
    path = build.build_refdist()
    assert path == _refdist_lib.LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("gsum_")}
    assert exported == declared
    lib = _refdist_lib.load_library()
    for name in declared:
        assert hasattr(lib, name)
    assert f"#define GSUM_REFDIST_LDS_SORT_MAX {16384}" in header
