"""The result record of the fused value paths across chunk seams and with k != 16 (run with ``-m gpu`` on an MI355X).

Every value path hands its results to the host as records of GS_RES_LEN doubles (kernels/common.hip.h) that ONE unpacker turns into
G / sum log L_ii / info, and the two one-workgroup paths share ONE chunk driver (gs_lml_one_block).  What that sharing can get wrong is an
index: a member of a later chunk unpacked to the place of an earlier one, a record read at stride k instead of the record's own 16, a
right-hand-side set index taken from the wrong chunk.  So every case here has k = 3 right-hand sides, members that all differ in their
hyperparameters, one member more than a launch holds, and the two members on either side of the seam not positive definite.

Reference in every case: THE SAME PATH called with one evaluation per call -- sum log L_ii and info equal bit for bit for every member (on
the grouped route sum log L_ii where info == 0: see there), G for every member with info == 0 (a failed member's G is unspecified).
Members that are not positive definite follow the recipe of
test_gpu_grad_pieces.test_a_member_that_is_not_positive_definite_in_the_middle_of_a_batch: two coincident points, a white-noise level of
1e-30, no nugget."""
import copy

import numpy as np
import pytest
from sklearn.gaussian_process.kernels import ConstantKernel as C, Matern, WhiteKernel

pytestmark = pytest.mark.gpu

import gsum_amd  # noqa: E402

K = 3


@pytest.fixture(scope="module")
def ctx():
    return gsum_amd.default_context(0)


@pytest.fixture(scope="module")
def lab():
    """The lab build (libgsum_hip_lab.so): same sources, the handle its neighbours use for the grouped route."""
    return gsum_amd.lab_context(0)


def problem(n, count, bad, n_sets=1):
    """X (n, 1) with rows 0 and n // 2 coincident, n_sets right-hand-side sets of k = 3 columns, and ``count`` flattened descriptors that
    all differ (length scale and amplitude); the members in ``bad`` carry white noise 1e-30 instead of 0.5 (and amplitude 1): not positive
    definite."""
    rng = np.random.RandomState(1000 * n + count)
    X = np.sort(rng.rand(n, 1) * (3.0 + 0.02 * n), axis=0)
    X[n // 2] = X[0]
    Zs = np.concatenate([rng.randn(n_sets, n, K - 1), np.ones((n_sets, n, 1))], axis=2)
    base = gsum_amd.describe_kernel(C(1.3) * Matern(0.7, nu=2.5) + WhiteKernel(0.5), 1)
    assert base.n_ops == 0 and base.white_noise == 0.5
    descs = []
    for i in range(count):
        dsc = copy.copy(base)
        dsc.length_scale[0] = 0.4 + 0.6 * i / count
        dsc.amplitude = 1.0 + 0.5 * ((7 * i) % 13) / 13.0
        if i in bad:
            dsc.white_noise = 1e-30
            dsc.amplitude = 1.0                # (the coincident rows' pivot is then 1 - 1 * 1: zero exactly, whatever the rounding of a square root)
        descs.append(dsc)
    return X, Zs, descs


def one_by_one(ctx, descs, members):
    """(G, sld, info) of ``members``, each from a call of its own on the resident inputs."""
    G, sld, info = np.empty((len(members), K, K)), np.empty(len(members)), np.empty(len(members), dtype=np.int64)
    for row, i in enumerate(members):
        g, s, f = ctx.lml_resident([descs[i]], 0.0)
        assert g.shape == (1, K, K)
        G[row], sld[row], info[row] = g[0], s[0], f[0]
    return G, sld, info


def check(label, got, want, members, bad, failed_sld=True):
    """Prints the figures, then asserts: sld and info of every member in ``members`` equal the reference's bits, G where info == 0; the
    members in ``bad`` -- and only they -- report info > 0.  failed_sld = False: sld is compared where info == 0 only."""
    G, sld, info = (np.asarray(a)[members] for a in got)
    Gw, sldw, infow = want
    ok = infow == 0
    print(f"{label}: {len(members)} members compared, {int((~ok).sum())} not positive definite (info {sorted(set(infow[~ok]))}), "
          f"sld differs at {members[np.flatnonzero(sld != sldw)].tolist()[:8]}, info at {members[np.flatnonzero(info != infow)].tolist()[:8]}, "
          f"G at {members[np.flatnonzero((G != Gw).any(axis=(1, 2)) & ok)].tolist()[:8]}")
    assert sorted(members[~ok].tolist()) == sorted(m for m in bad if m in set(members.tolist())), (label, members[~ok])
    assert np.array_equal(info, infow), label
    assert np.array_equal(sld, sldw) if failed_sld else np.array_equal(sld[ok], sldw[ok]), label
    assert np.array_equal(G[ok], Gw[ok]), label
    assert np.isfinite(G[ok]).all() and np.isfinite(sld[ok]).all() and (np.abs(G[ok]).sum(axis=(1, 2)) > 0).all(), label


SMALL_N, SMALL_COUNT, SMALL_BAD = 5, 4097, (4095, 4096)


@pytest.fixture(scope="module")
def small(ctx):
    """The small case's inputs and its reference, computed once: every member alone on set 0, every odd member alone on set 1
    (n = 5 <= 128: option small_path keeps a call of one on k_lml_small)."""
    X, Zs, descs = problem(SMALL_N, SMALL_COUNT, SMALL_BAD, n_sets=2)
    every, odd = np.arange(SMALL_COUNT), np.arange(1, SMALL_COUNT, 2)
    ctx.set_inputs(X, Zs[0])
    ref0 = one_by_one(ctx, descs, every)
    ctx.set_inputs(X, Zs[1])
    ref1 = one_by_one(ctx, descs, odd)
    return X, Zs, descs, ref0, ref1


def test_small_path_one_past_the_chunk_of_4096(ctx, small):
    """n = 5, 4097 evaluations: gs_lml_small launches 4096 workgroups of k_lml_small, then one; members 4095 and 4096 -- the last of the
    first launch, the only one of the second -- are not positive definite."""
    X, Zs, descs, ref0, _ = small
    ctx.set_inputs(X, Zs[0])
    check("small", ctx.lml_resident(descs, 0.0), ref0, np.arange(SMALL_COUNT), SMALL_BAD)


def test_small_path_with_two_sets_alternating_across_the_chunk(ctx, small):
    """The same call through gsum_lml_resident_sets, member i on right-hand-side set i % 2: the second launch reads its set index from
    the second chunk of set_of (member 4096: set 0; its neighbour 4095: set 1)."""
    X, Zs, descs, ref0, ref1 = small
    set_of = np.arange(SMALL_COUNT) % 2
    want = [a.copy() for a in ref0]
    for w, r in zip(want, ref1):
        w[1::2] = r
    assert not np.array_equal(want[0][:2], ref0[0][:2])              # (the sets do differ)
    ctx.set_inputs_sets(X, Zs)
    check("small, two sets", ctx.lml_resident_sets(descs, set_of, 0.0), want, np.arange(SMALL_COUNT), SMALL_BAD)


def test_medium_path_one_past_the_cap_of_512(ctx):
    """n = 129 (the smallest order that leaves the small path: np = 256, two diagonal blocks), 513 evaluations: gs_lml_medium launches 512
    workgroups of k_lml_medium, then one; members 511 and 512 are not positive definite.  Reference: EVERY member in a call of one, which
    option medium_min_batch = 1 keeps on k_lml_medium."""
    n, count, bad = 129, 513, (511, 512)
    X, Zs, descs = problem(n, count, bad)
    ctx.set_inputs(X, Zs[0])
    try:
        ctx.set_option("medium_min_batch", 1)
        want = one_by_one(ctx, descs, np.arange(count))
        got = ctx.lml_resident(descs, 0.0)
    finally:
        ctx.set_option("medium_min_batch", -1)
        ctx.set_option("release_scratch", 1)
    check("medium", got, want, np.arange(count), bad)


def test_grouped_route_against_the_single_slot_route(lab):
    """n = 300, 7 evaluations with medium_path = 0: one call takes the grouped route (gs_lml_wave: k_finalize_g's records, unpacked after
    the last round), a call of one the single-slot route (gs_eval_enqueue / gs_eval_harvest: k_finalize's record).  Member 3 is not
    positive definite; its sum log L_ii is not compared: on these routes k_finalize[_g] sums per-block partials, and a block that fails
    never writes its own, so the record holds what the workspace held before -- a failed member's sld is as unspecified as its G."""
    n, count, bad = 300, 7, (3,)
    X, Zs, descs = problem(n, count, bad)
    lab.set_inputs(X, Zs[0])
    try:
        lab.set_option("medium_path", 0)
        assert count >= lab.get_option("wave_min") > 1
        want = one_by_one(lab, descs, np.arange(count))
        got = lab.lml_resident(descs, 0.0)
    finally:
        lab.set_option("medium_path", 1)
    check("grouped / single", got, want, np.arange(count), bad, failed_sld=False)
