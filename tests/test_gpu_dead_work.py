"""The dead work the grouped batch schedule no longer touches on the GPU.  Option wave_env: the panel solves' waves
of row groups that the kernel build left all zero return before they load a row.  Option wave_far_plan: a far update's workgroups run a
list of its live tiles, and those behind the count leave at once.  On the banded, holed and dense inputs of tests/zero_skip_cases.py
every member of a batch still equals its single evaluation bit for bit, the factor left in the workspaces has the BITS of the launches
with both options off (int64 views: signs of zeros included), and the counters show that the banded inputs stop loading and listing
and the dense one does not."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import gsum_amd

import zero_skip_cases as zc

pytestmark = pytest.mark.gpu

LAB_OPTIONS = ("medium_path", "wave_groups", "wave_size", "wave_skip_zero", "wave_env", "wave_far_plan", "wave_depth")


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
        ctx.set_option("wave_panel_wg4", 4)               # (write-only options: their defaults)
        ctx.set_option("wave_cohort_min", 4)


@functools.lru_cache(maxsize=None)
def _descs(name):
    return tuple(gsum_amd.describe_kernel(k, 1) for k in zc.cases()[name]["kernels"])


_single_cache = {}


def _singles(ctx, name):
    """(G, sld, info) of every kernel of the case as a call of its own: the single-factorisation schedule, which has neither flags nor
    envelope.  Once per case."""
    if name not in _single_cache:
        c = zc.cases()[name]
        ctx.set_inputs(c["X"], c["Z"])
        out = [ctx.lml_resident([d], c["nugget"]) for d in _descs(name)]
        _single_cache[name] = tuple(np.concatenate([o[i] for o in out]) for i in range(3))
    return _single_cache[name]


def _batch(ctx, name, profile=False):
    c = zc.cases()[name]
    ctx.set_inputs(c["X"], c["Z"])
    if profile:
        ctx.set_option("profile_gemm", 1)
        ctx.kernel_profile()
    out = ctx.lml_resident(list(_descs(name)), c["nugget"])
    prof = None
    if profile:
        prof = ctx.kernel_profile()
        ctx.set_option("profile_gemm", 0)
    return out, prof


def _assert_equal(got, want):
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])


@pytest.mark.parametrize("env,plan", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("name", list(zc.cases()))
def test_batch_equals_single_evaluations(lab, name, env, plan):
    want = _singles(lab, name)
    assert np.all(want[2] == 0)
    lab.set_option("wave_env", env)
    lab.set_option("wave_far_plan", plan)
    assert (lab.get_option("wave_env"), lab.get_option("wave_far_plan")) == (env, plan)
    _assert_equal(_batch(lab, name)[0], want)


def _lower_bits(a):
    return np.ascontiguousarray(a[np.tril_indices(a.shape[0])]).view(np.int64)


@pytest.mark.parametrize("name", ["a", "d", "f272", "e", "h"])
def test_untouched_means_untouched(lab, name):
    """The lower triangle of the factor (with the solved right-hand-side rows) that the schedule leaves in the workspaces: the same
    BITS with both options on and both off -- a wave or a workgroup that returns early is one that stored nothing."""
    n_desc = len(_descs(name))
    assert lab.get_option("wave_env") == 1 and lab.get_option("wave_far_plan") == 1
    on, _ = _batch(lab, name)
    f_on = [_lower_bits(lab.wave_factor(i)) for i in range(n_desc)]
    lab.set_option("wave_env", 0)
    lab.set_option("wave_far_plan", 0)
    off, _ = _batch(lab, name)
    f_off = [_lower_bits(lab.wave_factor(i)) for i in range(n_desc)]
    _assert_equal(on, off)
    for a, b in zip(f_on, f_off):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", list(zc.cases()))
def test_the_counters(lab, name):
    c = zc.cases()[name]
    _, prof = _batch(lab, name, profile=True)
    groups, loaded = prof["panel_gemm"]["panel_groups"], prof["panel_gemm"]["panel_groups_loaded"]
    bulk = prof["bulk_update"]
    print(name, "panel_groups", groups, "loaded", loaded, "tiles", bulk["tiles"], "run", bulk["tiles_run"], "listed", bulk["tiles_listed"])
    assert bulk["tiles_listed"] == bulk["tiles_run"] > 0
    n_desc, np_ = len(_descs(name)), -(-c["X"].shape[0] // 256) * 256
    assert groups == n_desc * sum((np_ + 16 - 256 * (s + 1)) // 16 for s in range(np_ // 256))
    assert 0 < loaded <= groups
    if name == "a":
        assert loaded < groups
    if name == "e":
        assert loaded == groups
        assert bulk["tiles_listed"] == bulk["tiles"]
    lab.set_option("wave_env", 0)
    lab.set_option("wave_far_plan", 0)
    _, prof = _batch(lab, name, profile=True)
    assert prof["panel_gemm"]["panel_groups_loaded"] == prof["panel_gemm"]["panel_groups"] == groups
    assert prof["bulk_update"]["tiles_listed"] == 0 and prof["bulk_update"]["tiles_run"] == bulk["tiles_run"]


def test_flags_off_is_the_dense_launches(lab):
    """wave_skip_zero = 0 stays what it was whatever the two options say: every panel wave loads (and solves), nothing is listed, and the
    factor has the bits of the same call with both options off."""
    n_desc = len(_descs("a"))
    lab.set_option("wave_skip_zero", 0)
    on, prof = _batch(lab, "a", profile=True)
    f_on = [_lower_bits(lab.wave_factor(i)) for i in range(n_desc)]
    assert prof["panel_gemm"]["panel_groups_loaded"] == prof["panel_gemm"]["panel_groups"] > 0
    assert prof["bulk_update"]["tiles_listed"] == 0 and prof["bulk_update"]["tiles_run"] == prof["bulk_update"]["tiles"]
    lab.set_option("wave_env", 0)
    lab.set_option("wave_far_plan", 0)
    off, _ = _batch(lab, "a")
    _assert_equal(on, off)
    for a, b in zip(f_on, [_lower_bits(lab.wave_factor(i)) for i in range(n_desc)]):
        np.testing.assert_array_equal(a, b)


def test_a_failing_member_in_the_group(lab):
    """(a), (e) and a member that is not positive definite in one group (the recipe of
    test_gpu_zero_skip.py::test_banded_dense_and_failing_members_in_one_call): info as in single evaluations, the neighbours bit-equal."""
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


def test_reused_workspaces(lab):
    """Dense, banded, dense, holed on the same workspaces: the envelope is set again before every round's builds, nothing stale is read."""
    c = zc.cases()["a"]
    dense = [gsum_amd.describe_kernel(k, 1) for k in zc.cases()["e"]["kernels"]]           # (on case (a)'s points: the same order, so the
    lab.set_inputs(c["X"], c["Z"])                                                           #  groups' workspaces are used again)
    want_dense = tuple(np.concatenate(x) for x in zip(*[lab.lml_resident([d], 1e-10) for d in dense]))
    assert np.all(want_dense[2] == 0)
    for name in ("dense", "a", "dense", "f272", "d", "dense", "f40", "a"):
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


@pytest.mark.parametrize("depth,wg4", [(1, 4), (2, 0), (4, 8), (4, 0), (2, 8), (1, 0), (1, 8), (2, 4), (4, 4)])
def test_macro_step_depths_and_panel_workgroup_shapes(lab, depth, wg4):
    lab.set_option("wave_depth", depth)
    lab.set_option("wave_panel_wg4", wg4)
    for name in ("a", "c", "f48", "g1040"):
        _assert_equal(_batch(lab, name)[0], _singles(lab, name))
