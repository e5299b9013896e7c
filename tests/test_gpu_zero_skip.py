"""The grouped batch schedule with zero flags and K windows (option wave_skip_zero) on the GPU: on banded,
holed and dense kernel matrices (tests/zero_skip_cases.py) every member of a batch equals its single evaluation -- the untouched
schedule -- bit for bit, the factor left in the workspaces equals the dense launches' under ==, and the tile counter shows that the
banded inputs skip and the dense one does not."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import gsum_amd
from gsum_amd.conjugate import lml_from_gram_batch

import zero_skip_cases as zc

pytestmark = pytest.mark.gpu

LAB_OPTIONS = ("medium_path", "wave_groups", "wave_size", "wave_skip_zero", "wave_depth")


@pytest.fixture()
def lab():
    """the lab context with the grouped schedule forced (no one-workgroup medium path); every option a test moves is put back"""
    ctx = gsum_amd.lab_context(0)
    old = {k: ctx.get_option(k) for k in LAB_OPTIONS}
    ctx.set_option("medium_path", 0)
    try:
        yield ctx
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)
        ctx.set_option("profile_gemm", 0)
        ctx.set_option("wave_panel_wg4", 4)
        ctx.set_option("wave_cohort_min", 4)


@functools.lru_cache(maxsize=None)
def _descs(name):
    return tuple(gsum_amd.describe_kernel(k, 1) for k in zc.cases()[name]["kernels"])


_single_cache = {}


def _singles(ctx, name):
    """(G, sld, info) of every kernel of the case as a call of its own: the single-factorisation schedule, which has no flags.  Once per case."""
    if name not in _single_cache:
        c = zc.cases()[name]
        ctx.set_inputs(c["X"], c["Z"])
        out = [ctx.lml_resident([d], c["nugget"]) for d in _descs(name)]
        _single_cache[name] = tuple(np.concatenate([o[i] for o in out]) for i in range(3))
    return _single_cache[name]


@functools.lru_cache(maxsize=None)
def _oracle_lml(name):
    from gsum_amd._cpu import CpuContext
    c = zc.cases()[name]
    cpu = CpuContext()
    cpu.set_inputs(c["X"], c["Z"])
    G, sld, info = cpu.lml_resident(list(_descs(name)), c["nugget"])
    assert np.all(info == 0)
    return lml_from_gram_batch(G, sld, c["X"].shape[0], 0.0, 0.0, 1, 1)


def _batch(ctx, name, profile=False):
    c = zc.cases()[name]
    ctx.set_inputs(c["X"], c["Z"])
    if profile:
        ctx.set_option("profile_gemm", 1)
        ctx.kernel_profile()
    out = ctx.lml_resident(list(_descs(name)), c["nugget"])
    prof = None
    if profile:
        prof = ctx.kernel_profile()["bulk_update"]
        ctx.set_option("profile_gemm", 0)
    return out, prof


def _assert_equal(got, want):
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])


@pytest.mark.parametrize("name", list(zc.cases()))
def test_batch_equals_single_evaluations(lab, name):
    c = zc.cases()[name]
    want = _singles(lab, name)
    assert np.all(want[2] == 0)
    got, prof = _batch(lab, name, profile=True)
    _assert_equal(got, want)
    print(name, "tiles", prof["tiles"], "tiles_run", prof["tiles_run"])
    assert prof["tiles"] > 0
    if c["dense"]:
        assert prof["tiles_run"] == prof["tiles"]
    elif c["halfwidth"] or c["holes"]:
        assert 0 < prof["tiles_run"] < prof["tiles"]
    else:
        assert 0 < prof["tiles_run"] <= prof["tiles"]


@pytest.mark.parametrize("name", list(zc.cases()))
def test_lml_within_1e_10_of_the_cpu_oracle(lab, name):
    """The batch's log-likelihoods against the CPU oracle's (scipy's Cholesky on scikit-learn's matrix), relative, bound 1e-10, on every
    case.  (The cases are conditioned so that the oracle itself is defined to that bound: tests/zero_skip_cases.py on the nugget of (b),
    (c) and (d), and test_the_cpu_reference_is_defined_to_the_bound_on_every_case in test_zero_skip_cpu.py.)"""
    c = zc.cases()[name]
    got, _ = _batch(lab, name)
    lml = lml_from_gram_batch(got[0], got[1], c["X"].shape[0], 0.0, 0.0, 1, 1)
    ref = _oracle_lml(name)
    rel = np.abs(lml - ref) / np.abs(ref)
    print(name, "lml rel", rel)
    assert np.all(rel <= 1e-10), rel


def test_banded_dense_and_failing_members_in_one_call(lab):
    """(a), (e) and a member that is not positive definite in one group: info as in single evaluations, the neighbours untouched."""
    from sklearn.gaussian_process.kernels import RBF
    c = zc.cases()["a"]
    kernels = [zc.cases()["a"]["kernels"][0], zc.cases()["e"]["kernels"][0], RBF(40.0), zc.cases()["a"]["kernels"][1], zc.cases()["e"]["kernels"][1]]
    descs = [gsum_amd.describe_kernel(k, 1) for k in kernels]
    lab.set_inputs(c["X"], c["Z"])
    singles = [lab.lml_resident([d], 0.0) for d in descs]
    assert singles[2][2][0] > 0 and all(s[2][0] == 0 for i, s in enumerate(singles) if i != 2)
    for groups, size in ((1, 8), (3, 8)):                                   # all five in one group; spread over three
        lab.set_option("wave_groups", groups)
        lab.set_option("wave_size", size)
        G, sld, info = lab.lml_resident(descs, 0.0)
        for i, s in enumerate(singles):
            assert info[i] == s[2][0]
            if i != 2:                                                      # (G and sld are undefined where info > 0)
                np.testing.assert_array_equal(G[i], s[0][0])
                assert sld[i] == s[1][0]


def test_dense_then_banded_then_dense_on_the_same_workspaces(lab):
    """Flags are never cleared: every flag a tile reads was written in the same round, whatever the workspace held before."""
    c = zc.cases()["a"]
    dense = [gsum_amd.describe_kernel(k, 1) for k in zc.cases()["e"]["kernels"]]           # (on case (a)'s points: the same order, so the
    lab.set_inputs(c["X"], c["Z"])                                                           #  groups' workspaces are used again)
    want_dense = tuple(np.concatenate(x) for x in zip(*[lab.lml_resident([d], 1e-10) for d in dense]))
    assert np.all(want_dense[2] == 0)
    for name in ("dense", "a", "dense", "f272", "d", "dense", "a"):
        if name == "dense":
            lab.set_inputs(c["X"], c["Z"])
            _assert_equal(lab.lml_resident(dense, 1e-10), want_dense)
        else:
            _assert_equal(_batch(lab, name)[0], _singles(lab, name))


def test_several_rounds_and_the_cohort_route(lab):
    c = zc.cases()["a"]
    kernels = (zc.cases()["a"]["kernels"] + zc.cases()["b"]["kernels"] + zc.cases()["c"]["kernels"] + zc.cases()["e"]["kernels"])[:13]
    descs = [gsum_amd.describe_kernel(k, 1) for k in kernels]
    lab.set_inputs(c["X"], c["Z"])
    singles = [lab.lml_resident([d], 1e-10) for d in descs]
    want = tuple(np.concatenate([s[i] for s in singles]) for i in range(3))
    assert np.all(want[2] == 0)
    lab.set_option("wave_size", 2)                                          # 13 evaluations on 3 x 2: three rounds
    _assert_equal(lab.lml_resident(descs, 1e-10), want)
    lab.set_option("wave_size", 1)                                          # two cohorts per group at the smallest size: 2 x (3 x 1) evaluations
    lab.set_option("wave_cohort_min", 2)
    _assert_equal(lab.lml_resident(descs[:6], 1e-10), tuple(w[:6] for w in want))
    _assert_equal(lab.lml_resident(descs, 1e-10), want)


@pytest.mark.parametrize("depth,wg4", [(1, 4), (2, 0), (4, 8), (4, 0), (2, 8)])
def test_macro_step_depths_and_panel_workgroup_shapes(lab, depth, wg4):
    lab.set_option("wave_depth", depth)
    lab.set_option("wave_panel_wg4", wg4)
    for name in ("a", "c", "f48", "g1040"):
        _assert_equal(_batch(lab, name)[0], _singles(lab, name))


def _lower_equal(a, b):
    low = np.tril_indices(a.shape[0])
    return bool(np.all(a[low] == b[low]))


@pytest.mark.parametrize("name", ["a", "d", "f272", "e", "h"])
def test_skip_off_against_on_outputs_equal_and_factor_equal(lab, name):
    """wave_skip_zero = 0 is the dense launches: same outputs, and the factor (with the solved right-hand-side rows) in the workspaces is
    == entry for entry -- zeros off the envelope may differ in sign, nothing else."""
    n_desc = len(_descs(name))
    assert lab.get_option("wave_skip_zero") == 1
    on, prof_on = _batch(lab, name, profile=True)
    f_on = [lab.wave_factor(i) for i in range(n_desc)]
    lab.set_option("wave_skip_zero", 0)
    assert lab.get_option("wave_skip_zero") == 0
    off, prof_off = _batch(lab, name, profile=True)
    f_off = [lab.wave_factor(i) for i in range(n_desc)]
    _assert_equal(on, off)
    assert prof_off["tiles_run"] == prof_off["tiles"] == prof_on["tiles"]
    for a, b in zip(f_on, f_off):
        assert _lower_equal(a, b)
        assert not np.isnan(a[np.tril_indices(a.shape[0])]).any()


def test_gradient_batch_reads_the_factor_the_skipping_schedule_left():
    from gsum_amd.kernels import describe_gradient, describe_kernel
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C
    ctx = gsum_amd.default_context(0)
    c = zc.cases()["a"]
    kernels = [C(1.0 + 0.1 * i) * RBF(ell) + WhiteKernel(1e-10, noise_level_bounds="fixed") for i, ell in enumerate((0.2, 0.19, 0.21, 0.2))]
    descs = [describe_kernel(k, 1) for k in kernels]
    prms = [describe_gradient(k, 1) for k in kernels]
    singles = [ctx.lml_grad(d, p, c["X"], c["Z"], 0.0) for d, p in zip(descs, prms)]
    assert all(s[2] == 0 for s in singles)
    G, sld, info, tr, H = ctx.lml_grad_batch(descs, prms, c["X"], c["Z"], 0.0)
    for i, s in enumerate(singles):
        assert info[i] == 0
        np.testing.assert_array_equal(G[i], s[0])
        assert sld[i] == s[1]
        np.testing.assert_array_equal(tr[i], s[3])
        np.testing.assert_array_equal(H[i], s[4])
