"""tests/pointwise_edges.py validated without a device: the coverage cases are what they claim to be (distinct counters, the planted
points, backend='cpu' reproduces the expected counts through credible_diagnostic), the one-hot identities hold on the long-double
truth, and in every likelihood case float64 sits within LOGLIKE_RTOL / 16 of the truth and backend='cpu' within LOGLIKE_RTOL."""
import numpy as np
import pytest

import gsum_amd as gm
import pointwise_edges as pe
from pointwise_common import LOGLIKE_RTOL, loglike_magnitude


# ---- 1. coverage ------------------------------------------------------------------------------------------------------------------
def test_coverage_shapes_are_the_launch_edges():
    shapes = set(pe.COVERAGE_SHAPES)
    assert {D for n, kp, D in shapes if (n, kp) == (257, 5)} == {1, 127, 128, 129, 256, 257}
    assert {(kp, D) for n, kp, D in shapes if n == 257 and kp != 5} == {(1, 129), (63, 129), (64, 128), (64, 129)}
    assert {n for n, kp, D in shapes if (kp, D) == (5, 129)} == {1, 63, 64, 65, 255, 256, 257, 524289}
    assert 524289 == 256 * 2048 + 1
    assert all((n, kp, D, 1) in pe.COVERAGE_CASES and (n, kp, D, kp) in pe.COVERAGE_CASES for n, kp, D in shapes)


def _slow_counts(case, data_cols):
    """the same counts one interval and one column at a time"""
    data = case.data[data_cols]
    out = np.zeros((case.D, case.kp), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for j in range(case.kp):
            y, l, s = data[:, j if data_cols > 1 else 0], case.loc[:, j], case.scale[:, j]
            for d in range(case.D):
                lower, upper = case.t_lo[d] * s + l, case.t_hi[d] * s + l
                out[d, j] = np.count_nonzero(lower < y) - np.count_nonzero((lower < y) & ~(y < upper))
    return out


@pytest.mark.parametrize("n,kp,D,data_cols", pe.COVERAGE_CASES)
def test_coverage_case(n, kp, D, data_cols):
    case = pe.coverage_case(n, kp, D)
    assert case.loc.shape == case.scale.shape == (n, kp) and case.t_lo.shape == case.t_hi.shape == (D,)
    assert sorted(case.data) == sorted({1, kp})
    table = case.counts(data_cols)
    assert case.data[data_cols].shape == (n, data_cols) and table.shape == (D, kp) and table.dtype == np.int64
    if n <= 4096:
        np.testing.assert_array_equal(table, _slow_counts(case, data_cols))
    if D > 2:                                                        # drawn one by one: neither sorted nor nested
        assert np.any(np.diff(case.t_lo) < 0) and np.any(np.diff(case.t_lo) > 0)
        assert np.any(np.diff(case.t_hi) < 0) and np.any(np.diff(case.t_hi) > 0)
        assert np.any((np.diff(case.t_lo) > 0) & (np.diff(case.t_hi) > 0))
    assert np.all(case.t_lo < case.t_hi)
    assert np.count_nonzero(case.t_lo == 0) == 1 and np.count_nonzero(case.t_hi == 0) == (D >= 3)
    if n >= pe.DISTINCT_MIN_N:
        assert case.distinct(data_cols)
        assert len({r.tobytes() for r in table}) == D and len({c.tobytes() for c in table.T}) == kp
        assert D < 127 or (table.max() > n // 2 and table.min() < n // 8)   # the counters span the range
    assert bool(case.plants) == (n >= pe.PLANT_MIN_N)
    if not case.plants:
        return
    assert [p[0] for p in case.plants] == list(pe.PLANTS) and len({p[1] for p in case.plants}) == len(pe.PLANTS)
    sensitive = 0
    for kind, i, j, d in case.plants:
        one, many = case.data[1][i, 0], case.data[kp][i, j]
        if kind == "data_nan":
            assert np.isnan(one) and np.isnan(many)
        elif kind == "loc_nan":
            assert np.isnan(case.loc[i, j])
        elif kind == "scale_nan":
            assert np.isnan(case.scale[i, j])
        elif kind in ("data_pinf", "data_ninf"):
            assert one == many == (np.inf if kind == "data_pinf" else -np.inf)
        elif kind == "scale_zero":
            assert np.all(case.scale[i] == 0)
        elif kind == "scale_negative":
            assert np.all(case.scale[i] < 0)
        elif kind == "scale_inf":
            assert np.all(np.isposinf(case.scale[i]))
        else:
            t = case.t_lo[d] if kind == "on_lower" else case.t_hi[d]
            bound = t * case.scale[i, j] + case.loc[i, j]
            assert one == many == bound                              # on the twice-rounded bound: outside
            fused = pe.fused_bound(t, case.scale[i, j], case.loc[i, j])
            sensitive += fused < bound if kind == "on_lower" else fused > bound
    assert sensitive >= 2, sensitive                                 # a bound rounded once would count these points
    # none of the non-finite points is ever counted, in any interval, whatever its other operands are
    for kind, i, j, d in case.plants:
        if kind in ("data_nan", "data_pinf", "data_ninf", "scale_zero", "scale_negative"):
            rows = slice(i, i + 1)
            got = pe.coverage_expected(case.loc[rows], case.scale[rows], case.data[1][rows], case.t_lo, case.t_hi)
            assert not got.any(), kind
    i = next(p[1] for p in case.plants if p[0] == "scale_inf")      # t = 0 against scale = inf: NaN bounds, never counted
    rows = slice(i, i + 1)
    z = [int(np.flatnonzero(case.t_lo == 0)[0])] + ([int(np.flatnonzero(case.t_hi == 0)[0])] if D >= 3 else [])
    assert not pe.coverage_expected(case.loc[rows], case.scale[rows], case.data[1][rows], case.t_lo[z], case.t_hi[z]).any()


def test_credible_diagnostic_cpu_is_the_expression():
    """backend='cpu' of the public call the device is compared with at n = 1025, D = 257: its counts are numpy's expression"""
    m, data, dobs = pe.credible_inputs("cpu")
    got = m.credible_diagnostic(data, dobs)
    assert got.shape == (257, 5)
    counts = m._coverage_counts(data[:, None], dobs)
    np.testing.assert_array_equal(got, counts / 1025)
    assert len({r.tobytes() for r in counts[1:-1]}) > 200            # not a trivial table


# ---- 2. one-hot rows -----------------------------------------------------------------------------------------------------------------
def test_onehot_background_is_an_exact_zero():
    """(+-1)^2 + (+-1)^2 = 2, log(2 / 2) = 0, log|1| + 1 * log 1 = 0: in float64 as in long double"""
    pe._require_extended()
    n = 1025
    d0, d1 = pe.onehot_signs(n)
    assert set(d0) == set(d1) == {-1.0, 1.0} and len({(a, b) for a, b in zip(d0, d1)}) == 4
    dy = np.stack([d0, d1], axis=1)
    for ratio, ref in ((1.0, 1.0), (np.ones(n), 1.0), (1.0, np.ones(n))):
        T, M = pe.truth_row(dy, pe.ONEHOT_ORDERS, ratio, ref, pe.ONEHOT_DF0, pe.ONEHOT_SCALE0)
        assert T == 0 and M == 0
    y = np.stack([d0, d0 + d1], axis=1)
    assert pe.f64_row(y, pe.ONEHOT_ORDERS, [True, True], np.ones(n), np.ones(n), 0.0, 1.0) == 0.0


@pytest.mark.parametrize("n", pe.ONEHOT_SIZES)
def test_onehot_calls_cover_the_positions(n):
    calls = pe.onehot_calls(n)
    P = pe.onehot_positions(n)
    assert [p for p, _ in calls] == P and all(len(qs) == pe.ONEHOT_G and p in qs for p, qs in calls)
    assert {qs.index(p) for p, qs in calls} == {0, 1, 2}             # the one-hot row rotates
    assert {q for _, qs in calls for q in qs} == set(P)
    assert n - 1 == (n - 1) // 1024 * 1024                          # the last point is alone in its segment
    thread = lambda i: (i // 1024, i % 256)                         # noqa: E731  (segment, lane): the points one thread of k_loglike adds
    assert all(thread(p) != thread(q) for p, qs in calls for q in qs if q != p)


@pytest.mark.parametrize("ratio_kind", pe.RATIO_KINDS)
@pytest.mark.parametrize("ref_kind", pe.REF_KINDS)
@pytest.mark.parametrize("n", pe.ONEHOT_SIZES[:2])
def test_onehot_identities_on_the_truth(n, ratio_kind, ref_kind):
    """the truth of a row is the truth of its planted point, or the long-double sum of its two planted points' truths"""
    pe._require_extended()
    single = {}

    def alone(point):
        if point not in single:
            y, ratios, refs, _ = pe.single_operands(point, ratio_kind, ref_kind)
            ratio, ref = pe.row_operands(ratios, refs, ref_kind, 0)
            single[point] = pe.truth_row(pe.differences(y), pe.ONEHOT_ORDERS, ratio, ref, pe.ONEHOT_DF0, pe.ONEHOT_SCALE0)[0]
        return single[point]

    shapes = set()
    for p, qs in pe.onehot_calls(n):
        dy = pe.differences(pe.onehot_y(n, p))
        ratios, refs, _, points = pe.onehot_operands(n, p, qs, ratio_kind, ref_kind)
        for g in range(pe.ONEHOT_G):
            ratio, ref = pe.row_operands(ratios, refs, ref_kind, g)
            T, _ = pe.truth_row(dy, pe.ONEHOT_ORDERS, ratio, ref, pe.ONEHOT_DF0, pe.ONEHOT_SCALE0)
            assert 1 <= len(points[g]) <= 2
            want = alone(points[g][0]) if len(points[g]) == 1 else alone(points[g][0]) + alone(points[g][1])
            assert T == want and T != 0, (p, qs, g)
            shapes.add(len(points[g]))
    per_row = ratio_kind == "Gn" or ref_kind == "Gn"
    assert shapes == ({1, 2} if per_row else {1})
    assert all(abs(alone(pt)) > 0.01 for pt in single)                # a planted point cannot pass for a background point


# ---- 3. the grid likelihood ----------------------------------------------------------------------------------------------------------
def test_regimes_are_the_issues():
    R = pe.REGIMES
    assert R["benign"].orders == tuple(range(6)) and R["benign"].excluded == (0,)
    assert len(R["one"].orders) - len(R["one"].excluded) == 1
    for name in ("sixty-four", "sixty-four/small"):
        assert R[name].orders == tuple(range(65)) and R[name].excluded == (0,) and R[name].sizes == pe.SIZES
    assert R["sixty-four"].fit_ratio == (0.8, 0.3) and R["sixty-four"].grid_ratios[0] == (0.7, 0.6)
    assert R["sixty-four/small"].fit_ratio == (0.3, 0.0) and R["sixty-four/small"].grid_ratios[0] == (0.05, 0.05)
    assert R["negative"].orders == tuple(range(-3, 4)) and R["negative"].excluded == ()
    assert all(a > 1 and a + b > 1 for a, b in R["negative"].grid_ratios)
    assert R["sparse"].orders == (0, 2, 3, 7, 40) and R["sparse"].excluded == (2,) and R["sparse"].df0 == 0
    assert pe.SIZES == (1, 255, 256, 257, 1023, 1024, 1025, 2049)
    assert R["benign"].sizes == R["sparse"].sizes == pe.SIZES + (65536, 65537)
    assert all(len({g for g in r.grid_ratios}) == 3 for r in R.values())


def test_small_ratio_row_reaches_1e40_and_stays_finite():
    p = pe.problem("sixty-four/small", 2049)
    c = gm.coefficients(p.y, ratio=p.ratios[0], ref=p.fit_ref, orders=p.orders)[:, p.mask]
    assert np.max(np.abs(c)) > 1e40 and np.all(np.isfinite(np.sum(c * c, axis=1)))


def test_excluded_middle_order_keeps_its_column_in_the_differences():
    """sparse: column 2 (order 3) minus column 1 (the excluded order 2), not minus column 0"""
    p = pe.problem("sparse", 257)
    assert list(p.kept) == [0, 3, 7, 40]
    np.testing.assert_array_equal(p.dy[:, 1], p.y[:, 2] - p.y[:, 1])
    assert np.all(p.dy[:, 1] != p.y[:, 2] - p.y[:, 0])


@pytest.mark.parametrize("name,n", pe.LIKELIHOOD_CASES)
def test_likelihood_case_float64_sits_inside_the_cap(name, n):
    pe._require_extended()
    p = pe.problem(name, n)
    cpu = p.model("cpu")
    worst = 0.0
    for g, (T, M, f64) in enumerate(pe.likelihood_truth(name, n)):
        assert np.isfinite(float(T)) and M > 0
        e_ref = pe.rel_error(f64, T, M)
        worst = max(worst, e_ref)
        assert e_ref <= pe.REF_CAP, (name, n, g, e_ref)
        got = cpu.log_likelihood(ratio=p.ratios[g])
        e_cpu = abs(float(pe.LD(cpu._constants()) - T - pe.LD(got))) / loglike_magnitude(cpu, p.ratios[g], None)
        assert e_cpu <= LOGLIKE_RTOL, (name, n, g, e_cpu)
    print(f"{name} n={n}: worst e_ref / eps = {worst / pe.EPS:.2f}")


@pytest.mark.parametrize("n,ratio_kind,ref_kind", pe.MODE_CASES)
def test_mode_case_float64_sits_inside_the_cap(n, ratio_kind, ref_kind):
    pe._require_extended()
    p, ratios, refs, _ = pe.mode_operands(n, ratio_kind, ref_kind)
    cpu = p.model("cpu")
    for g, (T, M, f64) in enumerate(pe.mode_truth(n, ratio_kind, ref_kind)):
        e_ref = pe.rel_error(f64, T, M)
        assert e_ref <= pe.REF_CAP, (n, ratio_kind, ref_kind, g, e_ref)
        ratio, ref = pe.row_operands(ratios, refs, ref_kind, g)
        got = cpu.log_likelihood(ratio=ratio, ref=ref)
        e_cpu = abs(float(pe.LD(cpu._constants()) - T - pe.LD(got))) / loglike_magnitude(cpu, ratio, ref)
        assert e_cpu <= LOGLIKE_RTOL, (n, ratio_kind, ref_kind, g, e_cpu)
    rows = [t[0] for t in pe.mode_truth(n, ratio_kind, ref_kind)]
    assert len(set(rows)) == 3                                       # a wrong row index cannot pass


def test_change_of_variables_counts_once_or_n_times():
    pe._require_extended()
    p = pe.problem("benign", 257)
    once, _ = pe.truth_row(p.dy, p.kept, 0.4, 2.0, p.df0, p.scale0)
    many, _ = pe.truth_row(p.dy, p.kept, np.full(257, 0.4), 2.0, p.df0, p.scale0)
    jac = np.log(pe.LD(2.0)) + pe.LD(int(np.sum(p.kept))) * np.log(pe.LD(0.4))
    assert abs(float(many - once - 256 * jac)) <= 1e-15 * abs(float(256 * jac))


@pytest.mark.parametrize("name", sorted(pe.class_cases()))
def test_classes_on_the_cpu(name):
    case = pe.class_cases()[name]
    ratios, refs, want = case[6:]
    with np.errstate(all="ignore"):
        got = pe.class_model(case, "cpu").log_likelihood_grid(ratios, refs)
    assert [pe.value_class(v) for v in got] == want
