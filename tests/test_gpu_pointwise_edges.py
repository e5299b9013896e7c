"""libgsum_pointwise.so on the cases of tests/pointwise_edges.py: k_coverage across its interval blocks, LDS table and strided tile
loop (exact counts), k_differences / k_loglike / k_loglike_rows on one-hot rows (bit for bit), and the grid likelihood against the
long-double truth in five order regimes (LOGLIKE_RTOL, unchanged).  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from conftest import record_parity

import gsum_amd as gm
import pointwise_edges as pe
from gsum_amd._pointwise_lib import MAX_ORDERS, DevicePointwise, load_library
from pointwise_common import LOGLIKE_RTOL

pytestmark = pytest.mark.gpu


# ---- 1. coverage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kp,D,data_cols", pe.COVERAGE_CASES)
def test_coverage_counts_are_exact(n, kp, D, data_cols):
    case = pe.coverage_case(n, kp, D)
    orders, mask = pe.coverage_handle_inputs(kp)
    with DevicePointwise(0, np.zeros((n, kp)), orders, mask) as dev:
        got = dev.coverage(case.loc, case.scale, case.data[data_cols], case.t_lo, case.t_hi)
        again = dev.coverage(case.loc, case.scale, case.data[data_cols], case.t_lo, case.t_hi)       # the counters start from zero each call
    assert got.dtype == np.int64 and got.shape == (D, kp)
    np.testing.assert_array_equal(got, case.counts(data_cols))
    np.testing.assert_array_equal(again, got)


def test_credible_diagnostic_257_intervals_through_the_public_call():
    hip, data, dobs = pe.credible_inputs("hip")
    cpu, _, _ = pe.credible_inputs("cpu")
    try:
        np.testing.assert_array_equal(hip.credible_diagnostic(data, dobs), cpu.credible_diagnostic(data, dobs))
    finally:
        hip.close()


def test_refusals():
    k = MAX_ORDERS + 1
    with pytest.raises(ValueError, match=f"between 1 and {MAX_ORDERS} orders must be kept, got {k}"):
        DevicePointwise(0, np.zeros((4, k)), np.arange(k), np.ones(k))
    with pytest.raises(ValueError, match=f"between 1 and {MAX_ORDERS} orders must be kept, got 0"):
        DevicePointwise(0, np.zeros((4, 3)), np.arange(3), np.zeros(3))
    with DevicePointwise(0, np.zeros((4, 3)), np.arange(3), np.ones(3)) as dev:
        a, t = np.zeros((4, 3)), np.zeros(2)
        for cols in (2, 4):
            with pytest.raises(ValueError):
                dev.coverage(a, a + 1, np.zeros((4, cols)), t, t + 1)
        # ... and the library's own check behind the binding's
        lib = load_library()
        from gsum_amd._sidelib import _d, _i64
        counts = np.zeros((2, 3), dtype=np.int64)
        rc = lib.gsum_pointwise_coverage(dev._handle(), _d(a), _d(a + 1), _d(np.zeros((4, 2))), 2, _d(t), _d(t + 1), 2, _i64(counts))
        assert rc != 0 and b"data_cols must be 1 or 3, got 2" in lib.gsum_pointwise_last_error()
        np.testing.assert_array_equal(dev.coverage(a, a + 1, np.zeros((4, 1)), t - 1, t + 1), np.full((2, 3), 4))   # the handle still works


# ---- 2. one-hot rows -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alone():
    """the raw output of an n = 1 handle that holds one planted point, by (point, ratio kind, ref kind); computed once"""
    cache, handles = {}, {}

    def get(point, ratio_kind, ref_kind):
        key = (point, ratio_kind, ref_kind)
        if key not in cache:
            y, ratios, refs, mode = pe.single_operands(point, ratio_kind, ref_kind)
            if point[:2] not in handles:
                handles[point[:2]] = DevicePointwise(0, y, pe.ONEHOT_ORDERS, [1, 1])
            cache[key] = handles[point[:2]].loglike_grid(ratios, refs, mode, pe.ONEHOT_DF0, pe.ONEHOT_SCALE0)[0]
        return cache[key]

    yield get
    for h in handles.values():
        h.free()


@pytest.fixture(scope="module")
def onehot_handles():
    """n -> [(p, qs, handle)]: the differences are planted at p, uploaded once for the eight modes"""
    made = {}

    def get(n):
        if n not in made:
            made[n] = [(p, qs, DevicePointwise(0, pe.onehot_y(n, p), pe.ONEHOT_ORDERS, [1, 1])) for p, qs in pe.onehot_calls(n)]
        return made[n]

    yield get
    for calls in made.values():
        for _, _, h in calls:
            h.free()


@pytest.mark.parametrize("ratio_kind", pe.RATIO_KINDS)
@pytest.mark.parametrize("ref_kind", pe.REF_KINDS)
@pytest.mark.parametrize("n", pe.ONEHOT_SIZES)
def test_onehot_rows_are_their_planted_points(n, ratio_kind, ref_kind, alone, onehot_handles):
    """Every background point adds exactly +0.0, so a row is its planted point's own output, or fl(a + b) of its two planted points',
    whatever the order of the sum: a point read from the wrong place, twice or not at all changes the bits."""
    for p, qs, dev in onehot_handles(n):
        ratios, refs, mode, points = pe.onehot_operands(n, p, qs, ratio_kind, ref_kind)
        got = dev.loglike_grid(ratios, refs, mode, pe.ONEHOT_DF0, pe.ONEHOT_SCALE0)
        for g in range(pe.ONEHOT_G):
            parts = [alone(pt, ratio_kind, ref_kind) for pt in points[g]]
            want = parts[0] if len(parts) == 1 else parts[0] + parts[1]
            assert np.isfinite(want) and want != 0
            assert got[g] == want, (n, ratio_kind, ref_kind, p, qs, g, float(got[g]), float(want))


def test_onehot_background_alone_is_plus_zero():
    n = 2049
    d0, d1 = pe.onehot_signs(n)
    with DevicePointwise(0, np.stack([d0, d0 + d1], axis=1), pe.ONEHOT_ORDERS, [1, 1]) as dev:
        for ratios, refs, mode in ((np.ones(3), np.ones(1), pe.REF_SCALAR), (np.ones((3, n)), np.ones((3, n)), pe.REF_ROW_POINTS)):
            got = dev.loglike_grid(ratios, refs, mode, pe.ONEHOT_DF0, pe.ONEHOT_SCALE0)
            assert np.all(got == 0) and not np.any(np.signbit(got))


# ---- 3. the grid likelihood against the truth ----------------------------------------------------------------------------------------
def _record(label, errs):
    e_dev, e_ref = max(e[0] for e in errs), max(e[1] for e in errs)
    record_parity(f"pointwise_edges/{label}", e_dev_over_eps=e_dev / pe.EPS, e_ref_over_eps=e_ref / pe.EPS, bound_over_eps=LOGLIKE_RTOL / pe.EPS)
    return e_dev


@pytest.mark.parametrize("name,n", pe.LIKELIHOOD_CASES)
def test_grid_against_the_truth(name, n):
    pe._require_extended()
    p = pe.problem(name, n)
    truth = pe.likelihood_truth(name, n)
    hip = p.model("hip")
    try:
        raw = hip._device_data().loglike_grid(p.ratios, p.fit_ref, pe.REF_POINTS, p.df0, p.scale0)
        grid = hip.log_likelihood_grid(p.ratios)
        rows = [hip.log_likelihood(ratio=p.ratios[g]) for g in range(3)]
    finally:
        hip.close()
    errs = [(pe.rel_error(raw[g], T, M), pe.rel_error(f64, T, M)) for g, (T, M, f64) in enumerate(truth)]
    for g, (e_dev, e_ref) in enumerate(errs):
        print(f"{name} n={n} row {g}: e_dev / eps = {e_dev / pe.EPS:.2f}, e_ref / eps = {e_ref / pe.EPS:.2f}")
    worst = _record(f"{name}/n{n}", errs)
    assert worst <= LOGLIKE_RTOL, (name, n, errs)
    np.testing.assert_array_equal(grid, hip._constants() - raw)
    for g in range(3):
        assert rows[g] == grid[g], (name, n, g)


@pytest.mark.parametrize("n,ratio_kind,ref_kind", pe.MODE_CASES)
def test_every_mode_against_the_truth(n, ratio_kind, ref_kind):
    """the eight ratio x ref modes where b > 0: ``g * n + i`` past the first segment, and at 65537 past the 64th partial"""
    pe._require_extended()
    p, ratios, refs, mode = pe.mode_operands(n, ratio_kind, ref_kind)
    truth = pe.mode_truth(n, ratio_kind, ref_kind)
    hip = p.model("hip")
    try:
        raw = hip._device_data().loglike_grid(ratios, refs, mode, p.df0, p.scale0)
        rows = [hip.log_likelihood(*pe.row_operands(ratios, refs, ref_kind, g)) for g in range(3)]
    finally:
        hip.close()
    errs = [(pe.rel_error(raw[g], T, M), pe.rel_error(f64, T, M)) for g, (T, M, f64) in enumerate(truth)]
    worst = _record(f"modes/n{n}_ratio{ratio_kind}_ref{ref_kind}", errs)
    assert worst <= LOGLIKE_RTOL, (n, ratio_kind, ref_kind, errs)
    for g in range(3):
        assert rows[g] == hip._constants() - raw[g], (n, ratio_kind, ref_kind, g)


@pytest.mark.parametrize("name", sorted(pe.class_cases()))
def test_classes_match_the_cpu(name):
    case = pe.class_cases()[name]
    ratios, refs, _ = case[6:]
    with np.errstate(all="ignore"):
        want = pe.class_model(case, "cpu").log_likelihood_grid(ratios, refs)
    hip = pe.class_model(case, "hip")
    try:
        got = hip.log_likelihood_grid(ratios, refs)
    finally:
        hip.close()
    assert [pe.value_class(v) for v in got] == [pe.value_class(v) for v in want], (got, want)
