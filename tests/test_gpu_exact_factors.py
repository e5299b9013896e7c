"""potrf, the triangular solves, the sweeps and the MFMA tiles on exactly representable factors (tests/exact_factors.py).

Every expected value is a closed form and every comparison but one is assert_array_equal: on these inputs no operation of the
factorisation or of its consumers rounds, on LAPACK (tests/test_exact_factors_cpu.py) or on the device (the derivation is in
exact_factors.py's docstring), so a dropped correction term, a tile that misses one K chunk on a ragged edge, or a stale read across a
stream hand-off that changes one entry shows as a mismatch -- also where every schedule shares the defect.  The one inexact output is
sum log L_ii, held to the derived bound eps (n + 1) ln 2 sum |e_i| (Design.sld_bound).  The sections follow DESIGN.md section 22."""
import itertools

import numpy as np
import pytest

import exact_factors as xf
from conftest import record_parity

pytestmark = pytest.mark.gpu

import gsum_amd as gm  # noqa: E402
from sklearn.gaussian_process.kernels import RBF  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    return gm.default_context(0)


@pytest.fixture(scope="module")
def lab():
    """A context on the LAB build of the library (include/gsum_hip_debug.h: schedule switches, the tile-level entry point)."""
    return gm.lab_context(0)


@pytest.fixture(scope="module")
def desc():
    return gm.describe_kernel(RBF(0.3), 1)


class options:
    """Set lab options for a block and put back what the context held before (read first: the lab context is shared by the process)."""

    def __init__(self, c, opts):
        self.c, self.opts = c, opts

    def __enter__(self):
        self.saved = {name: self.c.get_option(name) for name in self.opts}
        for name, value in self.opts.items():
            self.c.set_option(name, value)

    def __exit__(self, *exc):
        for name, value in self.saved.items():
            self.c.set_option(name, value)


# ---- 1. every operator, product context -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,part", xf.OPERATOR_CASES)
def test_operators_exact(ctx, n, part):
    xf.check_operators(ctx, xf.design(n, part), record=record_parity)


# ---- 2. every schedule of one factorisation, lab context -------------------------------------------------------------------------------
def _grid(**axes):
    return [dict(zip(axes, v)) for v in itertools.product(*axes.values())]


SCHEDULES = {
    "host": [dict(chain_persist=0, **g) for g in _grid(lookahead=(1, 0), chain_fused=(0, 1), la_depth2=(0, 1))],
    "lazy": [dict(chain_persist=0, lookahead=0, lazy_min_np=1024, lazy_far=f) for f in (0, 1, 2)],
    "chain": [dict(chain_persist=1, **g) for g in _grid(chain_rows=(256, 512), chain_lazy=(0, 1, 2))],
    "deep": [dict(chain_persist=1, chain_deep=1, chain_deep_rows=0, chain_depth=dp) for dp in (2, 4)],
}


@pytest.mark.parametrize("family", list(SCHEDULES))
@pytest.mark.parametrize("n", xf.SCHEDULE_ORDERS)
def test_schedules_exact(lab, n, family):
    """L and G against the expectation -- not against another schedule -- for every schedule of the family, twice each (a hand-off
    race would show on some run).  The options are set before the upload: the padded order is fixed at allocation."""
    d = xf.design(n, "rand", 2)
    Z = xf.operands(n, 5, 7)
    d.check(Z=Z)
    want_chain = family in ("chain", "deep")
    aborts = lab.get_option("chain_aborts")
    for opts in SCHEDULES[family]:
        with options(lab, opts):
            for _ in range(2):
                M = xf.check_factor(lab, d)
                try:
                    xf.check_gram(lab, M, d, Z)
                finally:
                    M.free()
            if want_chain:
                assert lab.get_option("chain_probe") == 1
                assert lab.get_option("chain_aborts") == aborts
                assert lab.get_option("chain_persist") == 1


# ---- 3. gs_fwd_sweep's three forms through sqrt_errors ---------------------------------------------------------------------------------
SWEEPS = _grid(predict_lookahead=(1, 0), predict_split=(0, 1), predict_lazy=(1, 0), predict_panel256=(1, 0), predict_depth=(2, 4))


def sweep_form(o, n, k):
    """which form of gs_fwd_sweep these options select at (n, k) with lazy_min_np = 1024 (host/api_operators.hip.h); n = 897 pads to
    np = 1024, T = 8: exactly on the look-ahead form's thresholds, where its one macro-step (depth 4) or two (depth 2) have no far launch"""
    np_ = -(-n // 256) * 256
    big = k >= 1024
    if big and o["predict_lookahead"] and o["predict_lazy"] and o["predict_panel256"] and np_ >= 1024 and np_ // 128 >= 8:
        return "lookahead"
    return "halves" if big and o["predict_split"] else "single"


@pytest.mark.parametrize("n,k", xf.SWEEP_CASES)
def test_sweep_forms_exact(lab, n, k):
    """E = L^-1 (Y - mean) and md2 for k integer columns through every combination of the sweep's options: the look-ahead sweep (far
    launches beside the chain stream's panels), the two half-sweeps and the single sweep, macro-steps of 2 and 4 pairs, k_panel256 or
    k_panel + GEMM + k_panel.  lazy_min_np = 1024 lets the grouped forms apply at these orders, and wave_deep_rows = 0 lets macro-steps
    of 4 pairs apply in the half-sweeps and the single sweep too (with the default of 3072 rows they are clipped to 2 at np <= 2304, and
    depth 4 would only be the look-ahead form's)."""
    d = xf.design(n, "rand", 3)
    Y = xf.operands(n, k, 9)
    mean = xf.operands(n, 1, 10)[:, 0]
    d.check(Y=Y, mean=mean)
    Ew = d.W(Y - mean[:, None])
    m2w = (Ew * Ew).sum(0)
    forms = set()
    M = xf.check_factor(lab, d)
    try:
        with options(lab, dict(lazy_min_np=1024, wave_deep_rows=0)):
            for o in SWEEPS:
                with options(lab, o):
                    forms.add(sweep_form(o, n, k))
                    E, m2 = lab.sqrt_errors(M, Y, mean, pivot=False, md2=True)
                    xf.eq(E, Ew)
                    xf.eq(m2, m2w)
    finally:
        M.free()
    assert forms == ({"single"} if k < 1024 else {"lookahead", "halves", "single"})


# ---- 4. info ---------------------------------------------------------------------------------------------------------------------------
INFO_SCHEDULES = {
    "product": None,
    "host": dict(chain_persist=0, lookahead=1, chain_fused=1),
    "lazy": dict(chain_persist=0, lookahead=0, lazy_min_np=1024, lazy_far=2),
    "chain": dict(chain_persist=1, chain_rows=256, chain_lazy=1),
    "deep": dict(chain_persist=1, chain_deep=1, chain_deep_rows=0, chain_depth=2),
}


@pytest.mark.parametrize("family", list(INFO_SCHEDULES))
@pytest.mark.parametrize("n", xf.INFO_ORDERS)
def test_info_exact(ctx, lab, n, family):
    """A_jj lowered by 4^e_j: pivot j is exactly 0; by 2 * 4^e_j: negative.  Both at every column: potrf == j + 1 exactly at the first
    and last column of micro-blocks, blocks and panels (even and odd columns of gs_potf2_16's pairs are refused by different
    expressions; an exact zero meets each); with two lowered diagonals the smaller index."""
    d = xf.design(n, "rand", 4)
    c, opts = (ctx, {}) if family == "product" else (lab, INFO_SCHEDULES[family])
    with options(c, opts):
        for cols, twice in xf.info_cases(n):
            xf.check_info(c, d, cols, twice)


@pytest.mark.parametrize("n", [385, 1025])
def test_pivot_guard_sits_where_common_says(ctx, n):
    """p <= gs_pivot_guard * A_jj with the default guard of 2 ulps (kernels/common.hip.h): a pivot of exactly 1 under A_jj = 2^51 + 1
    is refused with info j + 1 (the threshold is 1 + 2^-51), under A_jj = 2^50 + 1 it is accepted and the factor is the design's."""
    g, j = xf.guard_design(n, True)
    M = ctx.upload(g.A)
    try:
        assert ctx.potrf(M) == j + 1
    finally:
        M.free()
    g, j = xf.guard_design(n, False)
    xf.check_factor(ctx, g).free()


# ---- 5. call sequences and the state contract -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", xf.SEQUENCE_ORDERS)
def test_call_sequences_exact(ctx, n):
    skipped = ctx.get_option("uploads_skipped")
    xf.check_sequences(ctx, n)
    assert ctx.get_option("uploads_skipped") > skipped          # (the sequences did meet the equal-input skip of the shared upload buffer)


def test_refusals(ctx, desc):
    xf.check_refusals(ctx, desc)


def test_predict_var_contract(ctx, desc):
    xf.check_predict_var_contract(ctx, desc)


# ---- 6. the tiles ---------------------------------------------------------------------------------------------------------------------
def _cases_of(test):
    """the argument tuples of an existing parametrised test, from its own marks"""
    marks = [m for m in test.pytestmark if m.name == "parametrize"]
    return [m.args[1] for m in marks]


def _tile_cases():
    import test_gpu_parity as tp
    (rect,) = _cases_of(tp.test_mfma_gemm_tiles)
    lower = _cases_of(tp.test_mfma_gemm_lower_tiles)            # two marks: (cfg, BM) and M
    cfgs = next(a for a in lower if isinstance(a[0], tuple))
    Ms = next(a for a in lower if not isinstance(a[0], tuple))
    return list(rect), [(cfg, BM, M) for (cfg, BM) in cfgs for M in Ms]


RECT_TILES, LOWER_TILES = _tile_cases()
BETA_SIGN = ((1, -1.0), (0, 1.0), (1, 1.0))


def _ints(rng, *shape):
    return rng.integers(-3, 4, size=shape).astype(float)


@pytest.mark.parametrize("cfg,M,N,K", RECT_TILES)
def test_tiles_exact(lab, cfg, M, N, K):
    """C <- beta C + sign A B^T on integer operands in [-3, 3] (|sums| <= 9 K + 3: exact in any order), every case of
    test_mfma_gemm_tiles: the whole matrix equals numpy's."""
    rng = np.random.default_rng([cfg, M, N, K])
    A, B, C = _ints(rng, M, K), _ints(rng, N, K), _ints(rng, M, N)
    for beta, sign in BETA_SIGN:
        xf.eq(lab.debug_gemm_nt(cfg, C, A, B, tri=False, beta=beta, sign=sign), beta * C + sign * (A @ B.T))


@pytest.mark.parametrize("cfg,BM,M", LOWER_TILES)
def test_lower_tiles_exact(lab, cfg, BM, M):
    """tri mode, every case of test_mfma_gemm_lower_tiles: the lower triangle equals numpy's, tiles wholly above the diagonal are
    untouched (the same slack rule as there: the 128 x 64 tile's partial tile row comes first on a ragged matrix)."""
    rng = np.random.default_rng([cfg, M])
    A, C = _ints(rng, M, 128), _ints(rng, M, M)
    low = np.tril(np.ones((M, M), dtype=bool))
    slack = 1 if (cfg == 7 and M % 128) else 0
    for beta, sign in BETA_SIGN:
        got = lab.debug_gemm_nt(cfg, C, A, A, tri=True, beta=beta, sign=sign)
        xf.eq(got[low], (beta * C + sign * (A @ A.T))[low])
        for bi in range(-(-M // BM)):
            for bj in range(-(-M // 128)):
                if bj * 128 > bi * BM + BM - 1 + 128 * slack:          # tile entirely above the diagonal
                    sl = (slice(bi * BM, min(M, (bi + 1) * BM)), slice(bj * 128, min(M, (bj + 1) * 128)))
                    xf.eq(got[sl], C[sl])
