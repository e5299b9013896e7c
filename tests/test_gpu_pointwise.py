"""gsum_amd.TruncationPointwise on backend='hip' (libgsum_pointwise.so): the reference's numbers of tests/golden/pointwise.json, the
device against backend='cpu' at the sizes the kernels are for, reproducibility, and one timing record."""
import time

import numpy as np
import pytest
import scipy.stats as st

from conftest import record_parity

import gsum_amd as gm  # noqa: E402
from pointwise_common import (LOGLIKE_RTOL, check_diagnostic, check_model, check_poc, check_scan, golden, loglike_magnitude,  # noqa: E402
                              random_problem)

pytestmark = pytest.mark.gpu

G = golden()
CPU_ELEMENTS = 1 << 23                  # n * G of the largest grid: the row-by-row cpu side stays within seconds


def _pair(n, df=0.6, scale=0.8, k=6):
    """the same seeded problem fitted on both backends"""
    y, ratio, ref, orders, excluded = random_problem(n, k=k)
    fit = lambda backend: gm.TruncationPointwise(df=df, scale=scale, excluded=excluded, backend=backend).fit(y, ratio=ratio, ref=ref, orders=orders)  # noqa: E731
    return fit("hip"), fit("cpu")


def test_fixture_proof_of_concept():
    record_parity("pointwise_poc_hip", **check_poc(G, "hip"))


def test_fixture_models():
    worst = dict(thin_rel=0.0, loglike_err_over_M=0.0)
    for rec in G["models"]:
        got = check_model(G, rec, "hip")
        worst = {k: max(v, got[k]) for k, v in worst.items()}
    record_parity("pointwise_models_hip", bound=LOGLIKE_RTOL, **worst)


def test_fixture_scan():
    record_parity("pointwise_scan_hip", bound=LOGLIKE_RTOL, **check_scan(G, "hip"))


def test_fixture_credible_diagnostic():
    worst = 0.0
    for rec in G["diagnostic"]:
        worst = max(worst, check_diagnostic(G, rec, "hip")["band_rel"])
    record_parity("pointwise_diagnostic_hip", D_CI="exact", band_rel=worst)


@pytest.mark.parametrize("kind", ["rows", "scalars"])
@pytest.mark.parametrize("rows", [1, 7, 1500])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 350, 8192, 1 << 20])
def test_grid_against_cpu(n, rows, kind):
    rows = max(1, min(rows, CPU_ELEMENTS // n))
    hip, cpu = _pair(n)
    rng = np.random.RandomState(n + rows)
    if kind == "rows":
        ratios, refs = rng.uniform(0.2, 0.6, (rows, n)), None
    else:
        ratios, refs = rng.uniform(0.2, 0.6, rows), rng.uniform(1, 3, rows)
    got, want = hip.log_likelihood_grid(ratios, refs), cpu.log_likelihood_grid(ratios, refs)
    M = np.array([loglike_magnitude(cpu, ratios[g], None if refs is None else refs[g]) for g in range(rows)])
    err = float(np.max(np.abs(got - want) / M))
    record_parity(f"pointwise_grid_n{n}_G{rows}_{kind}", err_over_M=err, bound=LOGLIKE_RTOL)
    assert got.shape == (rows,) and np.all(np.isfinite(got))
    assert err <= LOGLIKE_RTOL, err
    hip.close()


@pytest.mark.parametrize("ratio_kind", ["scalar", "array"])
@pytest.mark.parametrize("ref_kind", ["default", "scalar", "array"])
def test_every_shape_combination_against_cpu(ratio_kind, ref_kind):
    n, rows = 350, 5
    hip, cpu = _pair(n, df=0, scale=1)
    rng = np.random.RandomState(5)
    ratios = rng.uniform(0.2, 0.6, rows) if ratio_kind == "scalar" else rng.uniform(0.2, 0.6, (rows, n))
    refs = None if ref_kind == "default" else rng.uniform(1, 3, rows) if ref_kind == "scalar" else rng.uniform(1, 3, (rows, n))
    got, want = hip.log_likelihood_grid(ratios, refs), cpu.log_likelihood_grid(ratios, refs)
    for g in range(rows):
        ratio, ref = ratios[g], None if refs is None else refs[g]
        M = loglike_magnitude(cpu, ratio, ref)
        assert abs(got[g] - want[g]) <= LOGLIKE_RTOL * M
        assert abs(hip.log_likelihood(ratio=ratio, ref=ref) - want[g]) <= LOGLIKE_RTOL * M
    hip.close()


@pytest.mark.parametrize("n", [1, 65, 8192, 1 << 20])
def test_coverage_against_cpu(n):
    hip, cpu = _pair(n)
    dobs = np.linspace(0, 1, 101)
    rng = np.random.RandomState(n)
    spread = 3 * np.median(cpu.dist_.kwds["scale"])
    for data in (cpu.y_masked_[:, -1] + spread * rng.standard_normal(n), cpu.y_masked_ + spread * rng.standard_normal(cpu.y_masked_.shape)):
        got, want = hip.credible_diagnostic(data, dobs), cpu.credible_diagnostic(data, dobs)
        assert got.shape == (101, cpu.y_masked_.shape[1])
        np.testing.assert_array_equal(got, want)
    if n >= 8192:
        assert 0 < want[50].min() and want[50].max() < 1                           # the case is not a trivial one
    hip.close()


def test_data_on_a_bound_is_outside():
    n = 1000
    hip, cpu = _pair(n)
    loc, scale = np.broadcast_arrays(cpu.dist_.kwds["loc"], cpu.dist_.kwds["scale"])
    for dob in (0.5, 0.95):
        for sign in (-1.0, 1.0):
            t = st.t(cpu.df_).ppf((1.0 + sign * dob) / 2)
            data = t * scale + loc                                                 # exactly the bound the interval is built from
            for m in (hip, cpu):
                np.testing.assert_array_equal(m.credible_diagnostic(data, [dob]), np.zeros((1, loc.shape[1])))
            inside = (t * (1 - 1e-6)) * scale + loc                                # a hair inside: every point counts
            for m in (hip, cpu):
                np.testing.assert_array_equal(m.credible_diagnostic(inside, [dob]), np.ones((1, loc.shape[1])))
    hip.close()


def test_reproducible_bits():
    n, rows = 8192, 300
    hip, _ = _pair(n)
    ratios = np.random.RandomState(1).uniform(0.2, 0.6, (rows, n))
    whole = hip.log_likelihood_grid(ratios)
    np.testing.assert_array_equal(hip.log_likelihood_grid(ratios), whole)
    halves = np.concatenate([hip.log_likelihood_grid(ratios[:130]), hip.log_likelihood_grid(ratios[130:])])
    np.testing.assert_array_equal(halves, whole)
    assert hip.log_likelihood(ratio=ratios[7]) == whole[7]
    data = hip.y_masked_[:, -1]
    dobs = np.linspace(0, 1, 101)
    np.testing.assert_array_equal(hip.credible_diagnostic(data, dobs), hip.credible_diagnostic(data, dobs))
    hip.close()


def test_timing_record():
    """Device time (HIP events, by phase) and wall time of the 1500-row scan at n = 8192 and of the coverage at n = 2^20 with
    D = 101, beside the numpy time of the same work.  Only correctness is asserted; the figures are a record."""
    hip, cpu = _pair(8192)
    ratios = np.random.RandomState(2).uniform(0.2, 0.6, (1500, 8192))
    hip.log_likelihood_grid(ratios[:8])                                            # first launch: code object load
    hip.device_times(reset=True)
    t0 = time.perf_counter()
    got = hip.log_likelihood_grid(ratios)
    scan_wall = time.perf_counter() - t0
    scan_ms = hip.device_times(reset=True)
    t0 = time.perf_counter()
    want = cpu.log_likelihood_grid(ratios)
    scan_numpy = time.perf_counter() - t0
    M = np.array([loglike_magnitude(cpu, ratios[g], None) for g in (0, 750, 1499)])
    assert np.max(np.abs(got - want)[[0, 750, 1499]] / M) <= LOGLIKE_RTOL
    hip.close()

    hip, cpu = _pair(1 << 20)
    dobs = np.linspace(0, 1, 101)
    data = cpu.y_masked_[:, -1] + 3 * np.median(cpu.dist_.kwds["scale"]) * np.random.RandomState(3).standard_normal(1 << 20)
    hip.credible_diagnostic(data[:], dobs[:2])
    hip.device_times(reset=True)
    t0 = time.perf_counter()
    got = hip.credible_diagnostic(data, dobs)
    cov_wall = time.perf_counter() - t0
    cov_ms = hip.device_times(reset=True)
    t0 = time.perf_counter()
    want = cpu.credible_diagnostic(data, dobs)
    cov_numpy = time.perf_counter() - t0
    np.testing.assert_array_equal(got, want)
    hip.close()
    record_parity("pointwise_timing", scan_rows=1500, scan_n=8192, scan_device_ms=scan_ms, scan_wall_s=scan_wall, scan_numpy_s=scan_numpy,
                  coverage_n=1 << 20, coverage_D=101, coverage_device_ms=cov_ms, coverage_wall_s=cov_wall, coverage_numpy_s=cov_numpy)
    print(f"[pointwise timing] scan 1500 x 8192: device {scan_ms} ms, wall {scan_wall:.4f} s, numpy {scan_numpy:.4f} s")
    print(f"[pointwise timing] coverage 2^20 x D=101: device {cov_ms} ms, wall {cov_wall:.4f} s, numpy {cov_numpy:.4f} s")
