"""The gradient pieces of gsum_lml_grad[_batch] -- trace_p = tr(R^-1 dR_p), H_p = V^T dR_p V, beside G and sum log L_ii -- against
long-double truth on every path that produces them (run with ``-m gpu`` on an MI355X): the one-workgroup kernel k_grad_small<TREE>
(n <= 128), the general path (k_set_identity, the U = L^-T sweep, k_upper_times_rows, the SYRK, k_grad_contract<TREE, R, SPLIT> with
k_grad_trace, k_grad_reduce1 / 2) and the batch entry point's slot pipeline, grouped route and 512-member chunks.

Bound (tests/grad_truth.py; validated without a device in tests/test_grad_pieces_cpu.py): with the normalised error
e(x) = max |x - truth| / (cond_2(R) S) of a piece,   e_dev <= 16 max(e_ref, eps)   for trace, H, G and sld, where e_ref is the float64 CPU
reference's error on the same inputs (<= 1.9 eps on every case).  Every shape runs twice -- WhiteKernel(0.5): cond < 1e3, where 16 eps cond
stays ten orders of magnitude under any structural error, and WhiteKernel(1e-6): rounding amplified by 1e4 ... 1e8 -- and with two kinds of
right-hand sides: random, Z = [randn(n, k - 1) | 1], and the selector Z = R[:, cols], for which V = e_cols and H_p[a, b] = dR_p[cols_a, cols_b]:
single entries of the kernel gradient (the last row, row 0, coincident points, a diagonal entry).  Every case's e_dev / eps and e_ref / eps
go to the parity record (conftest.record_parity); the worst ratios per path are in DESIGN.md section 9."""
import warnings

import numpy as np
import pytest

from conftest import record_parity

pytestmark = pytest.mark.gpu

import gsum_amd  # noqa: E402
from gsum_amd._cpu import cpu_context  # noqa: E402

import grad_truth as gt  # noqa: E402

EPS = gt.EPS
PIECES = ("trace", "H", "G", "sld")


@pytest.fixture(scope="module")
def ctx():
    return gsum_amd.default_context(0)


@pytest.fixture(scope="module")
def lab():
    """The lab build (libgsum_hip_lab.so): the schedule switches and batch routes chosen below are not part of the product ABI."""
    return gsum_amd.lab_context(0)


def describe(kern, d):
    return gsum_amd.describe_kernel(kern, d), gsum_amd.kernels.describe_gradient(kern, d)


def reference(desc, prm, X, rhs, nugget=gt.NUGGET):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")                       # (scikit-learn's own 0 / 0 at coincident points of Matern-1/2)
        return cpu_context().lml_grad(desc, prm, X, rhs, nugget)


def judge(label, T, name, dev, ref, record=True):
    """Errors of the device's and the reference's pieces against the truth T for right-hand sides ``name``; records them and returns the
    list of pieces over the bound (empty: fine) with the worst ratio e_dev / max(e_ref, eps)."""
    G, sld, info, tr, H = dev
    assert info == 0 and ref[2] == 0, (label, info, ref[2])
    e_dev = gt.piece_errors(T, name, G, sld, tr, H)
    e_ref = gt.piece_errors(T, name, ref[0], ref[1], ref[3], ref[4])
    ratios = {p: e_dev[p] / max(e_ref[p], EPS) for p in PIECES}
    if record:
        record_parity(f"grad_pieces/{label}/{name}", cond=T.cond, **{f"e_dev_{p}_eps": e_dev[p] / EPS for p in PIECES},
                      **{f"e_ref_{p}_eps": e_ref[p] / EPS for p in PIECES}, **{f"ratio_{p}": ratios[p] for p in PIECES})
    over = [f"{label}/{name}/{p}: e_dev {e_dev[p] / EPS:.3g} eps, e_ref {e_ref[p] / EPS:.3g} eps, ratio {ratios[p]:.3g} > {gt.BOUND:g}"
            for p in PIECES if not ratios[p] <= gt.BOUND]
    return over, ratios


@pytest.mark.parametrize("case,run,white", gt.CASE_RUNS, ids=gt.CASE_RUN_IDS)
def test_pieces_against_truth(ctx, case, run, white):
    """One evaluation (HipContext.lml_grad, default options) of every case of the matrix: n = 1 ... 128 in one workgroup (flat d = 1, 2, 8
    and trees), n = 129 ... 513 on the general path (two rows per wave for flat kernels: every odd n leaves the last wave half empty; one
    row per wave for trees), k = 1, 5, 16, RBF and Matern 5/2, 3/2, 1/2 with and without amplitude, free and fixed white noise, additive
    constant, coincident points under Matern-1/2, RationalQuadratic, ExpSineSquared, C * DotProduct, Exponentiation, a product of two leaves
    and the 17-operation four-leaf sum."""
    kern, X, R, dK, Z, Zs, cols, T = gt.case_truth(case, run, white)
    desc, prm = describe(kern, case.d)
    assert (desc.n_ops > 0) == case.path.endswith("tree") and len(prm) == dK.shape[2]
    over = []
    for name, rhs in (("random", Z), ("selector", Zs)):
        dev = ctx.lml_grad(desc, prm, X, rhs, gt.NUGGET)
        over += judge(f"{case.id}-{run}", T, name, dev, reference(desc, prm, X, rhs))[0]
    assert not over, "\n".join(over)


@pytest.mark.parametrize("n", [129, 257, 383])
def test_forms_of_one_evaluation_are_bit_identical_at_small_orders(lab, n):
    """grad_split x grad_interleave x chain_persist at the orders just past the one-workgroup kernel and on both sides of the second block
    column (test_single_gradient_evaluation_forms_are_bit_identical starts at 700): the split contraction + k_grad_trace, the fused
    contraction, the sweep enqueued between or behind the factorisation's steps -- every combination returns the default's bits, for the
    flat kernel and the tree of that order."""
    names = ("grad_split", "grad_interleave", "chain_persist")
    persist0 = lab.get_option("chain_persist")
    try:
        for case in [c for c in gt.CASES if c.n == n and c.path.startswith("general")]:
            kern, X, R, dK, Z, Zs, cols, T = gt.case_truth(case, "amplified", gt.WHITE_AMPLIFIED)
            desc, prm = describe(kern, case.d)
            for v, name in zip((1, 1, persist0), names):
                lab.set_option(name, v)
            want = lab.lml_grad(desc, prm, X, Z, gt.NUGGET)
            assert want[2] == 0
            for combo in [(s, i, c) for s in (0, 1) for i in (0, 1) for c in (0, 1)]:
                for v, name in zip(combo, names):
                    lab.set_option(name, v)
                got = lab.lml_grad(desc, prm, X, Z, gt.NUGGET)
                for a, b in zip(got, want):
                    assert np.array_equal(np.asarray(a), np.asarray(b)), (case.id, combo)
    finally:
        lab.set_option("grad_split", 1)
        lab.set_option("grad_interleave", 1)
        lab.set_option("chain_persist", persist0)


# ---- the batch entry point ----------------------------------------------------------------------------------------------------------
_BATCH = {}


def batch_truths(case, run, white, m, step, nugget=gt.NUGGET):
    """m members of a batch: the case's kernel at theta + step * i * (1, -1, 1, ...) -- every member has other hyperparameter values, so a
    mix-up between members shows -- with each member's truth for the shared right-hand sides (random, and the selector of member 0)."""
    key = (case.id, case.dup, run, m, step, nugget)
    if key not in _BATCH:
        base = case.kernel(white)
        X, Z, cols = case.inputs()
        sign = np.where(np.arange(len(base.theta)) % 2 == 0, 1.0, -1.0)
        members, Zs = [], None
        for i in range(m):
            kern = base.clone_with_theta(base.theta + step * i * sign)
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                K, dK = kern(X, eval_gradient=True)
            R = K + nugget * np.eye(case.n)
            if Zs is None:
                Zs = np.ascontiguousarray(R[:, cols])
            T = gt.pieces_truth(R, dK)
            gt.add_rhs(T, "random", Z)
            gt.add_rhs(T, "selector", Zs)
            T.Rinv = T.L = T.dR = None
            members.append((kern, T))
        _BATCH[key] = (X, Z, Zs, members)
    return _BATCH[key]


def check_batch(label, lab, case, X, rhs_by_name, members, nugget=gt.NUGGET, record=lambda i: True, skip=()):
    descs, prms = zip(*[describe(kern, case.d) for kern, _ in members])
    over, worst = [], {}
    for name, rhs in rhs_by_name.items():
        G, sld, info, tr, H = lab.lml_grad_batch(list(descs), list(prms), X, rhs, nugget)
        for i, (kern, T) in enumerate(members):
            if i in skip:
                continue
            o, ratios = judge(f"{label}/member{i}", T, name, (G[i], sld[i], int(info[i]), tr[i], H[i]),
                              reference(descs[i], prms[i], X, rhs, nugget), record=record(i))
            over += o
            for p in PIECES:
                worst[p] = max(worst.get(p, 0.0), ratios[p])
    record_parity(f"grad_pieces/{label}/worst", members=len(members), **{f"ratio_{p}": worst[p] for p in PIECES})
    assert not over, "\n".join(over[:20])


BATCH_257 = gt.Case("batch_flat", 257, 2, 5, "C(1.3) * Matern([0.7, 1.1], nu=2.5) + W(WHITE) + C(0.2)")
BATCH_200 = gt.Case("batch_flat", 200, 1, 5, "C(1.3) * RBF(0.7) + W(WHITE)")
BATCH_5 = gt.Case("batch_flat", 5, 1, 5, "C(1.3) * Matern(0.7, nu=2.5) + W(WHITE)")


@pytest.mark.parametrize("run,white", gt.RUNS, ids=[r for r, _ in gt.RUNS])
@pytest.mark.parametrize("route", ["grouped", "slots"])
def test_batch_of_three_at_257_on_both_routes(lab, route, run, white):
    """Three kernels at n = 257 on the grouped-factorisation route (gs_grad_batch_wave: wave_min = 2) and on the slot pipeline
    (grad_batch_wave = 0; both keep the fused contraction k_grad_contract<false, 2, false>): every member against its own truth."""
    X, Z, Zs, members = batch_truths(BATCH_257, run, white, 3, 0.07)
    wave_min = lab.get_option("wave_min")
    try:
        lab.set_option("wave_min", 2)
        lab.set_option("grad_batch_wave", 1 if route == "grouped" else 0)
        check_batch(f"batch257-{route}-{run}", lab, BATCH_257, X, dict(random=Z, selector=Zs), members)
    finally:
        lab.set_option("wave_min", wave_min)
        lab.set_option("grad_batch_wave", 1)


@pytest.mark.parametrize("run,white", gt.RUNS, ids=[r for r, _ in gt.RUNS])
def test_batch_of_two_at_200(lab, run, white):
    """Two kernels at n = 200 (one block column; below the grouped route's orders: the slot pipeline with default options)."""
    X, Z, Zs, members = batch_truths(BATCH_200, run, white, 2, 0.07)
    check_batch(f"batch200-{run}", lab, BATCH_200, X, dict(random=Z, selector=Zs), members)


@pytest.mark.parametrize("run,white", gt.RUNS, ids=[r for r, _ in gt.RUNS])
def test_batch_of_513_at_5_crosses_the_chunk_of_512(lab, run, white):
    """513 kernels at n = 5: gs_grad_small launches 512 workgroups, then one.  EVERY member against its own truth (the long-double evaluation
    costs a millisecond at this order), each with other hyperparameter values; members 0, 511 and 512 are recorded one by one."""
    X, Z, Zs, members = batch_truths(BATCH_5, run, white, 513, 0.002)
    check_batch(f"batch5x513-{run}", lab, BATCH_5, X, dict(random=Z), members, record=lambda i: i in (0, 511, 512))


@pytest.mark.parametrize("case,route", [(BATCH_5, "small"), (BATCH_200, "slots"), (BATCH_257, "slots"), (BATCH_257, "grouped")],
                         ids=["n5-one-workgroup", "n200-slots", "n257-slots", "n257-grouped"])
def test_a_member_that_is_not_positive_definite_in_the_middle_of_a_batch(lab, case, route):
    """Members 0 and 2 as above; member 1 has a white-noise level of 1e-30 on points two of which coincide, and no nugget: its factorisation
    stops (info > 0), its gradient pieces are zero, and its neighbours are as correct as without it."""
    dup = gt.Case(case.path, case.n, case.d, case.k, case.expr, dup=True)
    X, Z, Zs, members = batch_truths(dup, "tight", gt.WHITE_TIGHT, 3, 0.07, nugget=0.0)
    bad = dup.kernel(1e-30)
    members = [members[0], (bad, None), members[2]]
    wave_min = lab.get_option("wave_min")
    try:
        lab.set_option("wave_min", 2)
        lab.set_option("grad_batch_wave", 1 if route == "grouped" else 0)
        descs, prms = zip(*[describe(kern, dup.d) for kern, _ in members])
        G, sld, info, tr, H = lab.lml_grad_batch(list(descs), list(prms), X, Z, 0.0)
        assert info[1] > 0 and info[0] == 0 and info[2] == 0, info
        assert not tr[1].any() and not H[1].any(), (tr[1], H[1])
        one = lab.lml_grad(descs[1], prms[1], X, Z, 0.0)             # ... and alone (gs_grad_single above n = 128)
        assert one[2] == info[1] and not one[3].any() and not one[4].any()
        check_batch(f"notpd-n{case.n}-{route}", lab, dup, X, dict(random=Z), members, nugget=0.0, skip=(1,))
    finally:
        lab.set_option("wave_min", wave_min)
        lab.set_option("grad_batch_wave", 1)
