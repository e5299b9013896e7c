"""The predictive pieces' and the series scaling's long-double truth (tests/predict_cases.py) and the bound of
tests/test_gpu_predict_truth.py, validated without a device on the cpu backend: the truth is consistent with itself; the plain float64
reference has a normalised error of at most REF_LIMIT eps on EVERY case of the device matrix, so  e_dev <= BOUND max(e_ref, eps)  is a bound
of rounding size; the cpu backend meets that bound itself; the bound catches the errors it is for; and the border-row memo sequence of the
GPU test runs on the cpu backend.  Run with -s to see every figure."""
import numpy as np
import pytest

import gsum_amd
from gsum_amd._cpu import cpu_context

import grad_truth as gt
import predict_cases as pc

EPS = pc.EPS


def test_long_double_is_extended_precision_and_the_matrix_covers_its_shapes():
    gt._require_extended()
    pc.check_shape_coverage()
    for regime in pc.REGIMES:
        assert (len(pc.series_configs(regime)) == len(pc.SERIES)) == (regime != "above_one")
    assert sum(len(pc.SERIES[c][2]) == pc.MAX_EXCLUDED for c in pc.SERIES) == 1 and any(pc.SERIES[c][3] != 1.0 for c in pc.SERIES)


@pytest.mark.parametrize("n,m,run,white", [(129, 9, "tight", gt.WHITE_TIGHT), (257, 17, "amplified", gt.WHITE_AMPLIFIED)])
def test_truth_is_consistent_with_itself(n, m, run, white):
    """R Rinv = I to long-double rounding; the three pieces are blocks of one symmetric matrix; cov's diagonal is colsumsq."""
    ctx = cpu_context()
    X, Xs, Z = pc.points(n, m)
    desc = gsum_amd.describe_kernel(pc.kernel(white), 2)
    R, Kst = ctx.kernel_matrix(desc, X, diag_add=pc.NUGGET), ctx.kernel_matrix(desc, Xs, X)
    T = pc.predict_truth(("cpu", n, run), R, Kst, Z)
    Rinv = pc._RINV[("cpu", n, run)][1]
    resid = float(np.abs(R.astype(pc.LD) @ Rinv - np.eye(n, dtype=pc.LD)).max())
    print(f"n{n}-{run}: cond {T.cond:.3g}  max |R Rinv - I| = {resid:.3g}")
    assert resid <= 1e-15 * T.cond
    assert float(np.abs(T.Gt - T.Gt.T).max()) <= 1e-17 * float(T.S.max()) * T.cond
    css, _ = T.piece("colsumsq")
    cov, _ = T.piece("cov")
    assert np.array_equal(np.diag(cov), css) and T.piece("VtW", [0])[0].shape == (m, 1)
    assert len({tuple(r) for r in Xs.tolist()}) == m and not np.array_equal(Z, Z[::-1])


@pytest.mark.parametrize("n,m,run,white", pc.SHAPE_RUNS, ids=pc.SHAPE_RUN_IDS)
def test_reference_error_and_cpu_backend_on_every_shape(n, m, run, white):
    """e_ref of numpy.linalg.cholesky / solve_triangular / einsum on every shape and both white levels is at most REF_LIMIT eps (the case is
    admissible); the cpu backend's predict_terms meets the device's bound in every call variant.  (The bit-exact properties -- symmetric cov,
    VtW columns independent of each other -- are the device's: BLAS picks another routine for one column than for sixteen.)"""
    T, e_ref, calls = pc.evaluate_pieces(cpu_context(), ("cpu", n, run), n, m, white)
    print(f"n{n}-m{m}-{run} cond {T.cond:.3g} e_ref / eps: " + "  ".join(f"{p} {v / EPS:.3f}" for p, v in e_ref.items()))
    assert np.isfinite(T.cond) and (run != "tight" or T.cond < 1e3)
    for piece, v in e_ref.items():
        assert np.isfinite(v) and v <= gt.REF_LIMIT * EPS, (piece, v / EPS)
    over, worst = pc.over_bound(f"n{n}-m{m}-{run}", e_ref, calls)
    print("   cpu backend e / eps: " + "  ".join(f"{p} {v / EPS:.3f}" for p, v in worst.items()))
    assert not over, "\n".join(over)


@pytest.mark.parametrize("regime", pc.REGIMES)
@pytest.mark.parametrize("entry,shape", pc.SERIES_ENTRIES, ids=pc.SERIES_ENTRY_IDS)
def test_series_reference_error_on_every_case(entry, shape, regime):
    """e_ref of gsum_amd.geometric_sum (through the cpu backend's three entry points) on every regime, series and shape: at most REF_LIMIT
    eps with nothing left out but the planted x == 1 entries, which are nan in the reference (series_errors asserts count and class)."""
    worst = 0.0
    for config in pc.series_configs(regime):
        A, vec, got = pc.series_call(cpu_context(), entry, shape, regime, config)
        e_dev, e_ref = pc.series_errors(config, A, vec, got)
        print(f"{entry}-{shape}-{regime}-{config}: planted {vec[4]}  e_ref {e_ref / EPS:.3f} eps  cpu backend {e_dev / EPS:.3f} eps")
        assert np.isfinite(e_ref) and e_ref <= gt.REF_LIMIT * EPS, (config, e_ref / EPS)
        assert e_dev <= gt.BOUND * max(e_ref, EPS)
        worst = max(worst, e_ref)
    assert worst > 0.0 or shape == (1, None)


def test_series_truth_matches_a_term_by_term_sum():
    """S(x) of the truth against the sum written out term by term in long double, for every finite series, on a grid of x in (-0.9, 1.9)."""
    x = np.linspace(-0.9, 1.9, 57)
    x = x[x != 1.0]
    one = np.ones(1)
    for config, (start, end, exc, factor) in pc.SERIES.items():
        if not np.isfinite(end):
            continue
        truth, scale, unit = pc.series_truth(config, np.ones((len(x), 1)), np.ones(len(x)), x, one, one)
        direct = sum((x.astype(pc.LD) ** e for e in range(start, int(end) + 1) if e not in exc), pc.LD(0) * x) * pc.LD(factor)
        err = np.abs(truth[:, 0] - direct) / scale[:, 0]
        assert not unit.any() and float(err.max()) <= 64 * float(np.finfo(pc.LD).eps), (config, float(err.max()))


def test_planted_entries_are_where_the_cases_say():
    """The planted ratios reach every shape that can hold them: x == 1 twice in a symmetric finite series (2.0 x 0.5), once in an infinite
    one (1.0 x 1.0) and in a cross matrix; x = 0, the 1e-6 ratio and the subnormal power are there from eight values up."""
    for config in pc.SERIES:
        finite = np.isfinite(pc.SERIES[config][1])
        for n in (255, 256, 257, 129):
            ref, ratio, _, _, planted = pc.vectors("mid", config, n)
            assert planted == (2 if finite else 1) and 0.0 in ratio and 1e-6 in ratio and 2.9e-3 in ratio
            x = np.outer(ratio, ratio)
            assert int((x == 1.0).sum()) == planted
            assert 0.1 <= np.abs(ref).min() and np.abs(ref).max() <= 10 and (ref > 0).any() and (ref < 0).any()
        assert pc.vectors("mid", config, 1)[4] == 0
        assert pc.vectors("mid", config, 257, 1)[4] == 0 and pc.vectors("mid", config, 3, 257)[4] == 1
        assert pc.vectors("mid", config, 129, 255)[4] == 1
    p61 = np.float64(2.9e-3 * 2.9e-3) ** 61
    assert 0.0 < p61 < np.finfo(float).tiny and np.float64(2.9e-3 * 2.9e-3) ** 60 >= np.finfo(float).tiny and np.float64(1e-12) ** 61 == 0.0


@pytest.mark.parametrize("config", pc.PREDICT_SERIES_CONFIGS)
@pytest.mark.parametrize("n,m", pc.PREDICT_SERIES)
def test_series_scaled_predictive_pieces_reference_error(n, m, config):
    """predict_terms(series=) on a factor of the series-scaled matrix: the scaled R and Kst of the cpu backend as exact inputs; e_ref <=
    REF_LIMIT eps, and the cpu backend meets the bound."""
    series = (pc.series_scale(config),) + pc.predict_series_vectors(config, n, m)
    T, e_ref, calls = pc.evaluate_pieces(cpu_context(), ("cpu-series", n, m, config), n, m, gt.WHITE_TIGHT, series=series,
                                         variants=pc.VARIANTS[2:], covs=(True,))
    print(f"series {config} n{n}-m{m} cond {T.cond:.3g} e_ref / eps: " + "  ".join(f"{p} {v / EPS:.3f}" for p, v in e_ref.items()))
    for piece, v in e_ref.items():
        assert np.isfinite(v) and v <= gt.REF_LIMIT * EPS, (piece, v / EPS)
    over, _ = pc.over_bound(f"series-{config}-n{n}-m{m}", e_ref, calls)
    assert not over, "\n".join(over)


MUTATIONS = ["last new point dropped from the sums", "one conditioning column left out of colsumsq", "VtW columns swapped",
             "excluded order below start subtracted", "cov not mirrored"]


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_the_bound_catches_the_errors_it_is_for(mutation):
    """The device errors the bound exists for, put into the float64 reference on the host (tight run): each exceeds BOUND max(e_ref, eps)."""
    n, m = 257, 17
    ctx = cpu_context()
    X, Xs, Z = pc.points(n, m)
    desc = gsum_amd.describe_kernel(pc.kernel(gt.WHITE_TIGHT), 2)
    R, Kst = ctx.kernel_matrix(desc, X, diag_add=pc.NUGGET), ctx.kernel_matrix(desc, Xs, X)
    T = pc.predict_truth(("cpu", n, "tight"), R, Kst, Z)
    css, vtw, cov = pc.reference_pieces(R, Kst, Z)
    good = T.errors(css, vtw, cov)
    if "excluded" in mutation:
        config = "3-inf-x2,4"
        A, vec, got = pc.series_call(ctx, "upload", (257, None), "mid", config)
        x = np.outer(vec[1], vec[1])
        with np.errstate(all="ignore"):
            bad = got - (np.outer(vec[0], vec[0]) * x ** 2) * A
        e_bad, e_ref = pc.series_errors(config, A, vec, bad)
        print(f"{mutation}: e = {e_bad / EPS:.3g} eps against e_ref {e_ref / EPS:.3g} eps")
        assert e_bad > gt.BOUND * max(e_ref, EPS)
        return
    if "last new point" in mutation:
        css = css.copy()
        css[m - 1] = css[m - 2]                                   # (row nrows - 1 read twice, stored to the wrong place)
        bad = T.errors(css, vtw, cov)
    elif "column left out" in mutation:
        from scipy.linalg import solve_triangular
        V = solve_triangular(np.linalg.cholesky(R), Kst.T, lower=True)
        bad = T.errors(np.einsum("ij,ij->j", V[:-1], V[:-1]), vtw, cov)
    elif "swapped" in mutation:
        bad = T.errors(css, vtw[:, ::-1], cov)
    else:
        bad = T.errors(css, vtw, np.tril(cov))
    ratios = {p: bad[p] / (gt.BOUND * max(good[p], EPS)) for p in bad}
    print(f"{mutation}: " + "  ".join(f"{p} {r:.3g} x the bound" for p, r in ratios.items()))
    assert max(ratios.values()) > 1.0


# ---- the border-row memo (the sequence is shared with the GPU test: predict_cases.memo_sequence) ------------------------------------------
@pytest.mark.parametrize("n", [129, 257])
def test_border_row_memo_sequence_on_the_cpu_backend(n):
    pc.memo_sequence(cpu_context(), n)
