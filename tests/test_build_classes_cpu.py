"""The designs of tests/build_classes.py, validated without a device: each puts enough entries of every class of the exp argument (in
range / subnormal band / far) into the kernel build's plain tiles, the row-pair groups its two wave-wide ballots decide on exist in both
tile geometries, and scikit-learn's own matrix -- the reference of tests/test_gpu_build_classes.py -- stays within that test's bound of the
long-double truth, so a failure there is the device's and not the design's.  Run with -s to see every count."""
import numpy as np
import pytest

import build_classes as bc
import grad_truth as gt


def test_long_double_is_extended_precision():
    """The truth needs exp(-745) as a NORMAL number with bits to spare: x87 extended (64-bit mantissa, 15-bit exponent)."""
    assert np.finfo(bc.LD).nmant >= 63 and np.finfo(bc.LD).minexp < -16000
    assert float(np.exp(bc.LD(-745.0)) / bc.LD(5e-324)) == pytest.approx(0.57125, rel=1e-3)


def test_class_limits_are_the_build_kernels_own():
    """The limits restated in build_classes.py against the source they restate, and against where exp really becomes subnormal / zero."""
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "gsum_amd", "csrc", "kernels", "build.hip.h")).read()
    assert "const bool far = x < -745.2;" in src and "const bool inr = fabs(x) < GS_EXP_INRANGE;" in src
    assert "if (!(fabs(x) < GS_EXP_INRANGE)) return exp(x);" in src                              # the branching form: the same limit
    assert src.count("#define GS_EXP_INRANGE") == 1 and "#define GS_EXP_INRANGE 0x1.61da04cbafe44p+9 " in src
    assert bc.FAR_LIMIT == -745.2 and bc.IN_RANGE_LIMIT == float.fromhex("0x1.61da04cbafe44p+9")
    assert np.exp(np.nextafter(bc.FAR_LIMIT, 0.0)) == 0.0 and np.exp(bc.FAR_LIMIT) == 0.0        # far: exactly zero, with room
    assert np.exp(-bc.IN_RANGE_LIMIT) > 1.99 * np.finfo(float).tiny                               # in range: normal (two times the smallest)
    # gs_base_is_zero's thresholds on the squared distance lie inside FAR for every family
    for s, arg in ((1490.5, -0.5 * 1490.5), (111100.0, -np.sqrt(111100.0) * bc.SQRT5), (185200.0, -np.sqrt(185200.0) * bc.SQRT3),
                   (555500.0, -np.sqrt(555500.0))):
        assert arg < bc.FAR_LIMIT, (s, arg)


@pytest.mark.parametrize("design", bc.DESIGNS, ids=bc.DESIGN_IDS)
def test_class_mix(design):
    """Condition 1: at least 10 % of the entries in range, at least 10 % far, at least 1000 in the band -- in kern(X) and in kern(X, Y)."""
    for cross in (False, True):
        E = design.entries(cross)
        inr, band, far = E.counts()
        total = inr + band + far
        print(f"{design.name} {'kern(X, Y)' if cross else 'kern(X)':10s} {E.cls.shape}: in range {inr}, band {band}, far {far} (off the diagonal)")
        assert inr >= 0.1 * total and far >= 0.1 * total and band >= 1000, (design.name, cross, inr, band, far)
        assert len(E.args) == (2 if design.name == "tree_rbf_rbf" else 1)


@pytest.mark.parametrize("design", bc.DESIGNS, ids=bc.DESIGN_IDS)
def test_group_coverage(design):
    """Condition 2, per tile geometry (k_build2's 32 x 128 tiles with row pairs (2 q, 2 q + 1) on kern(X) and kern(X, Y); the fused path's
    128 x 128 tiles with pairs (r, r + 4)), over the row-pair groups of plain tiles: at least one group is far throughout (the first ballot
    skips it) and at least one holds a band lane beside a far lane (the second ballot recomputes single lanes).  The shuffled design exists
    for the opposite of the first: no diagonal structure, so groups that are far throughout cannot be asked of it -- it must instead hold
    all three classes in nearly every group."""
    for geometry, c in bc.group_counts(design).items():
        print(f"{design.name} {geometry:17s}: {c['groups']} row-pair groups in plain tiles, {c['all_far']} far throughout, "
              f"{c['band_and_far']} with band and far lanes, {c['all_three']} with all three classes")
        assert c["groups"] > 0 and c["band_and_far"] >= 1, (design.name, geometry, c)
        if design.shuffle:
            assert c["all_three"] >= 0.6 * c["groups"], (design.name, geometry, c)
        else:
            assert c["all_far"] >= 1, (design.name, geometry, c)


@pytest.mark.parametrize("design", bc.DESIGNS, ids=bc.DESIGN_IDS)
def test_reference_within_the_bound(design):
    """Condition 3: scikit-learn's kern(X) and kern(X, Y) against the long-double truth -- far entries exactly the far value (the class is
    defined by the float64 exponential being zero: the unrounded product p exp(x) of a Matern entry is up to 8e-320 there, and no float64
    evaluation of scikit-learn's formula returns it), in-range entries within 4 ulp, band entries within 4 ulp + 4 subnormal spacings of
    the exponential times its factor; printed: the worst fraction of the bound, and the worst exponential's error in subnormal spacings
    where the subnormal term governs."""
    for cross in (False, True):
        E, K = design.entries(cross), design.sklearn(cross)
        far = E.cls == bc.FAR
        np.testing.assert_array_equal(K[far], E.far_value)
        err = np.abs(K.astype(bc.LD) - E.truth)
        bound = E.bound(K, E.truth.astype(float))
        live = ~far
        frac = float(np.max(err[live] / bound[live]))
        sub = E.cls == bc.BAND
        sub &= E.sub_scale >= np.spacing(np.abs(K))                   # the subnormal term governs
        spacings = float(np.max(err[sub] / E.sub_scale[sub])) if sub.any() else 0.0
        print(f"{design.name} {'kern(X, Y)' if cross else 'kern(X)':10s}: worst error {frac:.3f} of the bound; worst exponential off by "
              f"{spacings:.3f} subnormal spacings")
        assert np.all(err[live] <= bound[live]), (design.name, cross, frac)
        if not cross:
            np.testing.assert_array_equal(E.truth[E.diag].astype(float), np.diag(K))


def test_closed_form_design_is_far_everywhere():
    """RBF(0.2) on 8 arange(n): every off-diagonal argument is at most -800, scikit-learn's matrix is exactly the identity."""
    from sklearn.gaussian_process.kernels import RBF
    for n in bc.CLOSED_FORM_NS:
        X = bc.CLOSED_FORM_STEP * np.arange(n)[:, None]
        assert -0.5 * (bc.CLOSED_FORM_STEP / 0.2) ** 2 < bc.FAR_LIMIT
        np.testing.assert_array_equal(RBF(0.2)(X), np.eye(n))


WIDE = [c for c in gt.CASES if c.path == "general_wide"]


@pytest.mark.parametrize("case", WIDE, ids=[c.id for c in WIDE])
def test_wide_gradient_cases_hold_every_class(case):
    """The wide grids among the gradient cases (tests/grad_truth.py): the arguments of their kernel matrix -- the gradient build's exp
    arguments -- meet conditions 1 and 2 as far as they apply to a kernel without tiles (k_grad_contract gives a wave whole rows, lanes
    64 columns apart): the class mix, rows whose 64-lane steps are far throughout, and steps that hold a band lane beside a far lane."""
    from sklearn.gaussian_process.kernels import Matern
    leaf = bc._leaves(case.kernel(gt.WHITE_TIGHT))[0][0]
    X, _, _ = case.inputs()
    s = ((X / leaf.length_scale)[:, None, 0] - (X / leaf.length_scale)[None, :, 0]) ** 2
    x = -np.sqrt(s) * bc.SQRT5 if isinstance(leaf, Matern) else -0.5 * s
    cls = np.where(x < bc.FAR_LIMIT, bc.FAR, np.where(np.abs(x) < bc.IN_RANGE_LIMIT, bc.IN_RANGE, bc.BAND))
    counts = [int(np.sum(cls == c)) for c in (bc.IN_RANGE, bc.BAND, bc.FAR)]
    steps = [cls[i, j0:j0 + 64] for i in range(case.n) for j0 in range(0, case.n - 63, 64)]
    all_far = sum(bool(np.all(v == bc.FAR)) for v in steps)
    mixed = sum(bool(np.any(v == bc.BAND) and np.any(v == bc.FAR)) for v in steps)
    print(f"{case.id}: in range {counts[0]}, band {counts[1]}, far {counts[2]}; 64-lane steps far throughout {all_far}, with band and far lanes {mixed}")
    assert counts[0] >= 0.1 * case.n ** 2 and counts[2] >= 0.1 * case.n ** 2 and counts[1] >= 1000
    assert all_far >= 1 and mixed >= 1
