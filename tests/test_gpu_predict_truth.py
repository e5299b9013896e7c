"""The predictive pieces of gsum_predict_terms[_series] -- colsumsq, V^T W, V^T V -- and the series scaling k_scale_series behind its three
entry points against long-double truth (run with ``-m gpu`` on an MI355X), at the shapes where the forward sweep changes shape (one to
five block columns) and where its kernels clamp or mask rows (m = 1 ... 129), and in the regimes where the geometric sum can go wrong
(x = 0, x < 0, x next to 1, x > 1, x == 1, powers that underflow, excluded orders in and out of range, GSUM_MAX_EXCLUDED of them).

Bound (tests/predict_cases.py; validated without a device in tests/test_predict_truth_cpu.py):  e_dev <= 16 max(e_ref, eps)  with the
normalised errors of tests/grad_truth.py.  The exact inputs of every truth are the DEVICE's own kernel matrices.  Every figure goes to the
parity record (conftest.record_parity); the worst per piece / regime are in DESIGN.md section 16.

Measured on an MI355X (e / eps): see DESIGN.md section 16."""
import numpy as np
import pytest

from conftest import record_parity

pytestmark = pytest.mark.gpu

import gsum_amd  # noqa: E402

import grad_truth as gt  # noqa: E402
import predict_cases as pc  # noqa: E402

EPS = pc.EPS


@pytest.fixture(scope="module")
def ctx():
    return gsum_amd.default_context(0)


@pytest.mark.parametrize("n,m,run,white", pc.SHAPE_RUNS, ids=pc.SHAPE_RUN_IDS)
def test_predictive_pieces_against_truth(ctx, n, m, run, white):
    """Default options.  rhs=None (k_rowsumsq), k = 1 and k = GSUM_MAX_RHS with a constant column (k_rowsumsq_vw), each with and without
    want_cov (the lower-tile V^T V and k_mirror_lower), on a factor of one to five block columns; cov bit-symmetric; V^T W's column 0 the
    same bits whether fifteen more columns come with it or none."""
    T, e_ref, calls = pc.evaluate_pieces(ctx, ("hip", n, run), n, m, white)
    over, worst = pc.over_bound(f"n{n}-m{m}-{run}", e_ref, calls)
    record_parity(f"predict_truth/n{n}-m{m}-{run}", cond=T.cond, **{f"e_dev_{p}_eps": worst[p] / EPS for p in pc.PIECES},
                  **{f"e_ref_{p}_eps": e_ref[p] / EPS for p in pc.PIECES})
    for piece, v in e_ref.items():
        assert v <= gt.REF_LIMIT * EPS, (piece, v / EPS)
    assert not over, "\n".join(over)
    pc.exact_properties(calls)


@pytest.mark.parametrize("regime", pc.REGIMES)
@pytest.mark.parametrize("entry,shape", pc.SERIES_ENTRIES, ids=pc.SERIES_ENTRY_IDS)
def test_series_scaling_against_truth(ctx, entry, shape, regime):
    """DeviceMatrix.scale_series on an uploaded symmetric matrix (n = 1, 255, 256, 257: the grid's 256-column edge, identity padding),
    kernel_matrix(X, series=) with diag_add and white noise (odd and even n: both paddings of the host build's leading dimension; bit for
    bit kernel_matrix_dev + scale_series) and kernel_matrix(X, Y, series=), every series of the regime.  The unscaled matrix of the same
    entry point is the exact input.  Non-finite exactly on the planted x == 1 entries, of the reference's class."""
    over, worst_dev, worst_ref = [], 0.0, 0.0
    for config in pc.series_configs(regime):
        A, vec, got = pc.series_call(ctx, entry, shape, regime, config)
        e_dev, e_ref = pc.series_errors(config, A, vec, got)
        worst_dev, worst_ref = max(worst_dev, e_dev), max(worst_ref, e_ref)
        assert e_ref <= gt.REF_LIMIT * EPS, (config, e_ref / EPS)
        if not e_dev <= gt.BOUND * max(e_ref, EPS):
            over.append(f"{entry}-{shape}-{regime}-{config}: e_dev {e_dev / EPS:.3g} eps, e_ref {e_ref / EPS:.3g} eps")
    n, m = shape
    record_parity(f"series_truth/{entry}/{regime}/n{n}" + (f"-m{m}" if m else ""), e_dev_eps=worst_dev / EPS, e_ref_eps=worst_ref / EPS)
    assert not over, "\n".join(over)


@pytest.mark.parametrize("n", [255, 257])
def test_scaled_matrix_keeps_its_identity_padding(ctx, n):
    """A positive definite matrix stays one under an infinite sum with positive ref (Schur product with the positive definite
    1 / (1 - ratio_i ratio_j), scaled by a positive diagonal): potrf of the scaled device matrix succeeds -- the rows beyond n still hold
    the identity -- and L L^T returns the scaled matrix to Cholesky's backward error  (n + 1) eps sqrt(a_ii a_jj)  (here with a factor 2)."""
    rng = np.random.RandomState(n)
    G = rng.randn(n, n + 8)
    A = G @ G.T / n + np.eye(n)
    ref, ratio = 0.5 + rng.rand(n), 0.3 + 0.4 * rng.rand(n)
    sc = pc.series_scale("0-inf")
    M = ctx.upload(A)
    try:
        M.scale_series(sc, ref, ratio)
        scaled = M.to_host()
        assert np.all(np.isfinite(scaled)) and ctx.potrf(M) == 0
        L = M.to_host()
    finally:
        M.free()
    assert float(np.abs(L @ L.T - scaled).max()) <= 2 * (n + 1) * EPS * float(np.diag(scaled).max())


@pytest.mark.parametrize("config", pc.PREDICT_SERIES_CONFIGS)
@pytest.mark.parametrize("n,m", pc.PREDICT_SERIES)
def test_series_scaled_predictive_pieces_against_truth(ctx, n, m, config):
    """gsum_predict_terms_series on a factor of the series-scaled matrix: R = kernel_matrix(series=) and Kst = kernel_matrix(Xs, X, series=)
    of the device as exact inputs, k = 16, want_cov."""
    series = (pc.series_scale(config),) + pc.predict_series_vectors(config, n, m)
    T, e_ref, calls = pc.evaluate_pieces(ctx, ("hip-series", n, m, config), n, m, gt.WHITE_TIGHT, series=series, variants=pc.VARIANTS[2:],
                                         covs=(True,))
    over, worst = pc.over_bound(f"series-{config}-n{n}-m{m}", e_ref, calls)
    record_parity(f"series_truth/predict_terms/mid/{config}-n{n}-m{m}", cond=T.cond, **{f"e_dev_{p}_eps": worst[p] / EPS for p in pc.PIECES},
                  **{f"e_ref_{p}_eps": e_ref[p] / EPS for p in pc.PIECES})
    for piece, v in e_ref.items():
        assert v <= gt.REF_LIMIT * EPS, (piece, v / EPS)
    assert not over, "\n".join(over)
    cov = calls[0][2][2]
    assert np.array_equal(cov, cov.T)


@pytest.mark.parametrize("n", [129, 257])
def test_border_row_memo_set_reused_and_invalidated(ctx, n):
    """gs_border_prepare / L->solved_k / L->solved_rhs: every call of the sequence returns the bits of the same call on a fresh factor."""
    pc.memo_sequence(ctx, n)
