"""The value record of the two one-workgroup kernels for n <= 128 (run with ``-m gpu`` on an MI355X).

k_lml_small and k_grad_small run ONE device function for the value steps (gs_small_value, kernels/fused.hip.h: kernel matrix, factorisation,
W^T, Gram matrix, record); the gradient kernel only adds a destination for the explicit block inverse.  So for the same inputs the two kernels
return the same record -- G, sum log L_ii, info -- bit for bit, on success and on failure, in both TREE instantiations (and the TREE = true
value kernel's flat branch returns what the TREE = false kernels do); and both equal the general path's (option small_path = 0 on the lab
context).
Every comparison is numpy.array_equal.
Orders: 1, 16 | 17 and 127 | 128 are the ends and both sides of a micro-block boundary (gs_diag_block factorises (n + 15) >> 4 micro-blocks)."""
import numpy as np
import pytest
from sklearn.gaussian_process.kernels import RBF, ConstantKernel as C, Matern, RationalQuadratic, WhiteKernel

pytestmark = pytest.mark.gpu

import gsum_amd  # noqa: E402
from gsum_amd.kernels import describe_gradient, describe_kernel  # noqa: E402

D = 2


@pytest.fixture(scope="module")
def lab():
    return gsum_amd.lab_context(0)


def described(kernels, d=D):
    return [describe_kernel(kk, d) for kk in kernels], [describe_gradient(kk, d) for kk in kernels]


def members():
    """Three flattened descriptors (the TREE = false kernels) and three trees (the TREE = true kernels), all different."""
    flat = C(1.4) * Matern([0.6, 1.1], nu=2.5) + WhiteKernel(1e-4)
    tree = C(0.9) * RBF(0.8) + C(0.4) * RationalQuadratic(length_scale=1.3, alpha=0.8) + WhiteKernel(1e-4)
    calls = {name: described([kern.clone_with_theta(kern.theta + 0.05 * i) for i in range(3)]) for name, kern in (("flat", flat), ("tree", tree))}
    assert [dd.n_ops > 0 for dd in calls["flat"][0]] == [False, False, False]
    assert [dd.n_ops > 0 for dd in calls["tree"][0]] == [True, True, True]
    return calls


@pytest.mark.parametrize("k", [1, 16])
@pytest.mark.parametrize("n", [1, 16, 17, 127, 128])
def test_value_and_gradient_kernels_return_the_same_record(lab, n, k):
    """lml_batch of three descriptors against lml_grad_batch of the same three against the general path, flat and tree.  A gradient call
    takes one hyperparameter structure, so it cannot hold a flat descriptor beside trees; a value call can, and there the flat member
    runs the TREE = true kernel's flat branch: tree | flat | tree must return the records the three have in their own calls."""
    rng = np.random.RandomState(100 * n + k)
    X = rng.rand(n, D) * (2.0 + 0.05 * n)
    Z = np.concatenate([rng.randn(n, k - 1), np.ones((n, 1))], axis=1)
    calls = members()
    records = {}
    try:
        for name, (descs, prms) in calls.items():
            lab.set_option("small_path", 0)
            general = lab.lml_batch(descs, X, Z, 1e-10)
            lab.set_option("small_path", 1)
            value = lab.lml_batch(descs, X, Z, 1e-10)
            grad = lab.lml_grad_batch(descs, prms, X, Z, 1e-10)
            assert value[0].shape == (3, k, k) and not np.asarray(value[2]).any(), (name, value[2])
            assert np.isfinite(value[0]).all() and np.isfinite(value[1]).all()
            assert not np.array_equal(value[0][0], value[0][2])                  # (the members do differ)
            for what, v, g, w in zip(("G", "sld", "info"), value, grad, general):
                assert np.array_equal(v, g), (name, what, "k_lml_small against k_grad_small")
                assert np.array_equal(v, w), (name, what, "k_lml_small against the general path")
            records[name] = value
        beside = [calls["tree"][0][0], calls["flat"][0][1], calls["tree"][0][2]]
        mixed = lab.lml_batch(beside, X, Z, 1e-10)
        lab.set_option("small_path", 0)
        mixed_general = lab.lml_batch(beside, X, Z, 1e-10)
    finally:
        lab.set_option("small_path", 1)
    for what, m, w, f, t in zip(("G", "sld", "info"), mixed, mixed_general, records["flat"], records["tree"]):
        assert np.array_equal(m, w), (what, "tree | flat | tree against the general path")
        assert np.array_equal(m[1], f[1]), (what, "the flat member beside trees")
        assert np.array_equal(m[0], t[0]) and np.array_equal(m[2], t[2]), (what, "the trees beside a flat member")


@pytest.mark.parametrize("n", [20, 33, 128])
def test_a_failed_member_gets_the_same_record_from_both_kernels(lab, n):
    """C * RBF without white noise or nugget, X[j] = X[j - 1]: not positive definite at column j -- in the first micro-block (j = 1), at a
    micro-block's first column (j = 16) and at the last point (j = n - 1, where info == n)."""
    kern = C(1.0) * RBF(1.0)
    desc, prm = describe_kernel(kern, 1), describe_gradient(kern, 1)
    Z = np.ones((n, 1))
    for j in (1, 16, n - 1):
        X = np.arange(n, dtype=float)[:, None] * 0.7
        X[j] = X[j - 1]
        try:
            lab.set_option("small_path", 0)
            _, sld_w, info_w = lab.lml_batch([desc], X, Z, 0.0)
            lab.set_option("small_path", 1)
            _, sld_v, info_v = lab.lml_batch([desc], X, Z, 0.0)
            _, sld_g, info_g, tr, H = lab.lml_grad(desc, prm, X, Z, 0.0)
        finally:
            lab.set_option("small_path", 1)
        print(f"n = {n}, j = {j}: info {int(info_v[0])} (k_lml_small) {info_g} (k_grad_small) {int(info_w[0])} (general path)")
        assert info_v[0] == info_g == info_w[0] and info_g > 0, (n, j, info_v, info_g, info_w)
        assert sld_v[0] == 0.0 and sld_g == 0.0, (n, j, sld_v, sld_g)
        assert not tr.any() and not H.any(), (n, j)
        if j == n - 1:
            assert info_g == n, (n, info_g)


def test_a_failed_middle_member_leaves_its_neighbours_alone(lab):
    """Three members, the middle one not positive definite (two coincident points, white noise 1e-30, amplitude 1: the pivot is 1 - 1 * 1):
    its neighbours' records -- gradient pieces included -- equal those of their single calls and the general path's."""
    n, k = 33, 3
    rng = np.random.RandomState(7)
    X = np.sort(rng.rand(n, 1) * 4.0, axis=0)
    X[1] = X[0]
    Z = np.concatenate([rng.randn(n, k - 1), np.ones((n, 1))], axis=1)
    good = C(1.3) * Matern(0.7, nu=2.5) + WhiteKernel(0.5)
    kernels = [good, C(1.0) * Matern(0.7, nu=2.5) + WhiteKernel(1e-30), good.clone_with_theta(good.theta + 0.1)]
    descs, prms = described(kernels, 1)
    try:
        lab.set_option("small_path", 0)
        general = lab.lml_batch(descs, X, Z, 0.0)
        lab.set_option("small_path", 1)
        value = lab.lml_batch(descs, X, Z, 0.0)
        grad = lab.lml_grad_batch(descs, prms, X, Z, 0.0)
    finally:
        lab.set_option("small_path", 1)
    assert value[2][1] == grad[2][1] == general[2][1] > 0 and value[1][1] == grad[1][1] == 0.0
    assert np.array_equal(value[2], general[2])
    for i in (0, 2):
        assert np.array_equal(value[0][i], general[0][i]) and value[1][i] == general[1][i], i
    assert not grad[3][1].any() and not grad[4][1].any()
    for i in (0, 2):
        one = lab.lml_batch([descs[i]], X, Z, 0.0)
        gone = lab.lml_grad(descs[i], prms[i], X, Z, 0.0)
        assert one[2][0] == 0
        for v, o in zip(value, one):
            assert np.array_equal(np.asarray(v)[i], np.asarray(o)[0]), i
        for g, o in zip(grad, gone):
            assert np.array_equal(np.asarray(g)[i], np.asarray(o)), i
        for v, g in zip(value, grad):
            assert np.array_equal(np.asarray(v)[i], np.asarray(g)[i]), i
