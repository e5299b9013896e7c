"""gsum_amd.TruncationPointwise on backend='cpu' and the helpers of gsum_amd.stats against the reference's own numbers
(tests/golden/pointwise.json), the grid likelihood against its row-by-row definition, the argument checks, and the export table of
libgsum_pointwise.so against include/gsum_pointwise.h (the library is cross-compiled for gfx950; no GPU is needed to read its symbols)."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.stats

from conftest import ROOT

import gsum_amd as gm  # noqa: E402
from pointwise_common import D, check_diagnostic, check_model, check_poc, check_scan, golden, random_problem  # noqa: E402

G = golden()


def test_notebook_proof_of_concept():
    check_poc(G, "cpu")


@pytest.mark.parametrize("i", range(len(G["models"])))
def test_fixture_models(i):
    check_model(G, G["models"][i], "cpu")


def test_fixture_covers_the_priors_and_shapes():
    seen = {(r["df"], r["scale"], r["fit_ratio"], r["fit_ref"]) for r in G["models"]}
    assert seen == {(df, s, a, b) for df, s in ((0, 1), (0.6, 0.8), (1, 1)) for a in ("scalar", "array") for b in ("scalar", "array")}
    assert G["orders"] == [0, 2, 3, 4, 5] and G["excluded"] == [0]
    assert D(G["scan"]["ratios"]).shape[0] >= 64


def test_fixture_scan():
    check_scan(G, "cpu")


@pytest.mark.parametrize("i", range(len(G["diagnostic"])))
def test_fixture_credible_diagnostic(i):
    check_diagnostic(G, G["diagnostic"][i], "cpu")


def test_helpers_against_the_fixture():
    for rec in G["hpd"]:
        got = gm.hpd(scipy.stats.beta, rec["alpha"], rec["a"], rec["b"])
        np.testing.assert_allclose(got, D(rec["interval"]), rtol=1e-9, atol=0)
    for rec in G["cartesian"]:
        np.testing.assert_array_equal(gm.cartesian(*[D(a) for a in rec["arrays"]]), D(rec["product"]))


@pytest.mark.parametrize("ratio_kind", ["scalar", "array"])
@pytest.mark.parametrize("ref_kind", ["default", "scalar", "array"])
def test_grid_is_its_rows_bit_for_bit(ratio_kind, ref_kind):
    n, rows = 37, 9
    y, ratio, ref, orders, excluded = random_problem(n)
    m = gm.TruncationPointwise(df=0.6, scale=0.8, excluded=excluded, backend="cpu").fit(y, ratio=ratio, ref=ref, orders=orders)
    rng = np.random.RandomState(3)
    ratios = rng.uniform(0.2, 0.6, rows) if ratio_kind == "scalar" else rng.uniform(0.2, 0.6, (rows, n))
    refs = None if ref_kind == "default" else rng.uniform(1, 3, rows) if ref_kind == "scalar" else rng.uniform(1, 3, (rows, n))
    grid = m.log_likelihood_grid(ratios, refs)
    assert grid.shape == (rows,) and grid.dtype == np.float64
    for g in range(rows):
        assert grid[g] == m.log_likelihood(ratio=ratios[g], ref=None if refs is None else refs[g])


def test_scalar_broadcast_quirk_of_the_change_of_variables():
    """scalar ratio with scalar ref counts the Jacobian once; the same numbers as (n,) arrays count it n times (models.py:1796)"""
    n = 11
    y, _, _, orders, excluded = random_problem(n)
    m = gm.TruncationPointwise(df=0, excluded=excluded, backend="cpu").fit(y, ratio=0.3, ref=2.0, orders=orders)
    once = m.log_likelihood(ratio=0.4, ref=2.0)
    many = m.log_likelihood(ratio=np.full(n, 0.4), ref=2.0)
    jac = np.log(2.0) + np.sum(orders[1:]) * np.log(0.4)
    assert many - once == pytest.approx(-(n - 1) * jac, rel=1e-12)
    assert m.log_likelihood_grid(np.array([0.4]), np.array([2.0]))[0] == once


def test_argument_checks(monkeypatch):
    y, ratio, ref, orders, excluded = random_problem(8)
    with pytest.raises(ValueError):
        gm.TruncationPointwise(backend="cpu").fit(y, ratio=ratio, ref=ref, orders=orders[:-1])
    with pytest.raises(ValueError):
        gm.TruncationPointwise(backend="cpu").log_likelihood()
    with pytest.raises(ValueError):
        gm.TruncationPointwise(backend="cpu").log_likelihood_grid(np.array([0.3]))
    with pytest.raises(ValueError):
        gm.TruncationPointwise(backend="cuda")
    m = gm.TruncationPointwise(backend="cpu").fit(y, ratio=ratio, ref=ref, orders=orders)
    for bad in (0.3, np.zeros((3, 7)), np.zeros((0, 8)), np.zeros((2, 8, 1))):
        with pytest.raises(ValueError):
            m.log_likelihood_grid(bad)
    with pytest.raises(ValueError):
        m.log_likelihood_grid(np.full(3, 0.3), refs=np.ones(4))
    with pytest.raises(ValueError):
        m.log_likelihood_grid(np.full(3, 0.3), refs=np.ones((3, 7)))
    monkeypatch.setenv("GSUM_BACKEND", "cpu")
    assert gm.TruncationPointwise().backend == "cpu"
    m1 = gm.TruncationPointwise().fit(y[:, 0], ratio=0.3)                       # 1-D y is one order
    assert m1.y_.shape == (8, 1) and m1.df_ == 2


def test_public_names():
    for name in ("TruncationPointwise", "hpd", "hpd_pdf", "median_pdf", "cartesian"):
        assert name in gm.__all__ and hasattr(gm, name)


def test_pointwise_library_exports_every_declared_symbol():
    """include/gsum_pointwise.h is the contract of libgsum_pointwise.so: every function it declares is exported and bound, nothing else."""
    from gsum_amd import _pointwise_lib, build
    header = open(os.path.join(ROOT, "include", "gsum_pointwise.h")).read()
    declared = set(re.findall(r"\b(gsum_pointwise_[a-z0-9_]+)\s*\(", header))
    assert declared and declared == set(_pointwise_lib.PROTOTYPES), declared ^ set(_pointwise_lib.PROTOTYPES)
    path = build.build_pointwise()
    assert path == _pointwise_lib.LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("gsum_")}
    assert exported == declared
    lib = _pointwise_lib.load_library()
    for name in declared:
        assert hasattr(lib, name)
    assert f"#define GSUM_POINTWISE_MAX_ORDERS {_pointwise_lib.MAX_ORDERS}" in header
    for i, name in enumerate(("SCALAR", "POINTS", "ROW_SCALAR", "ROW_POINTS")):
        assert f"#define GSUM_POINTWISE_REF_{name} {i}" in header
