"""The device variogram's tile, chunk, curve-group, cache and LDS edges on the lattice of tests/vario_lattice.py: exact closed forms
for the pair stage, and the cov sums against the mpmath truth stored in tests/golden/vario_lattice_truth.json (no mpmath here).
Run with -m gpu on an MI355X.

Tolerances are derived, never measured (vario_lattice.Truth.atol; the pair stage's in test_pair_stage_sums_against_fsum)."""
import math

import numpy as np
import pytest

import gsum_amd as gm
import vario_lattice as vl
from conftest import load_golden
from gsum_amd._vario_lib import DeviceVariogram

pytestmark = pytest.mark.gpu

VF, CF = vl.VAR_FACTOR, vl.CORR_FACTOR
N = 600
EDGE = vl.EDGE_BINS


@pytest.fixture(scope="module")
def golden():
    cases = load_golden("vario_lattice_truth.json")["cases"]
    for name, (n, nc, variant, _) in vl.CASES.items():                # the model's bits on this machine are the fixture's
        gt = vl.model_gt(n, nc, variant)
        assert vl.gt_digest(gt) == cases[name]["gt_sha256"], name
        if "gt" in cases[name]:
            np.testing.assert_array_equal(gt, vl.A(cases[name]["gt"]))
    return {name: vl.Truth(rec) for name, rec in cases.items()}


@pytest.fixture(scope="module")
def smooth():
    """The N = 600 lattice with 5 smooth random curves: (object, z)"""
    X, bounds = vl.lattice(N)
    z = np.random.RandomState(5).standard_normal((5, N)).cumsum(axis=1) / np.sqrt(N)
    v = gm.VariogramFourthRoot(X, z, bounds, backend="hip")
    yield v, z
    v.close()


def device(n, nc, n_bounds=None, points=None):
    """DeviceVariogram of the lattice with nc indicator curves (of ``points``, default the first nc points)"""
    X, bounds = vl.lattice(n, n_bounds)
    points = list(range(nc)) if points is None else points
    return DeviceVariogram(0, X, np.eye(n)[points], bounds), points


def check_pair_stage(dev, n, points):
    nbin = len(dev.counts)
    np.testing.assert_array_equal(dev.counts, vl.counts_exact(n, nbin))
    np.testing.assert_array_equal(dev.h_sum, vl.h_sum_exact(n, nbin))
    np.testing.assert_array_equal(dev.dij_sum, vl.indicator_dij_exact(n, points, nbin))


def check_against_truth(got, truth, requests, nc=None, label=""):
    """got (n_requests, nc) within the derived tolerance of the truth's first nc curves; prints the worst error / tolerance"""
    nc = got.shape[1] if nc is None else nc
    worst = 0.
    for r, (a, b) in enumerate(requests):
        want, tol = truth.row(a, b).sum[:nc], truth.atol(a, b)[:nc]
        err = np.abs(got[r, :nc] - want)
        if truth.row(a, b).M:
            worst = max(worst, float(np.max(err / tol)))
        assert np.all(err <= tol), (label, (a, b), got[r, :nc], want, err, tol)
    print(f"{label}: worst |device - truth| / atol = {worst:.3f}")


# ---- pair stage ------------------------------------------------------------------------------------------------------------------
def test_pair_stage_exact_on_the_lattice():
    """z = eye(600): dij_sum[k, a] = [a >= k] + [a + k < N] pins the membership of every point in every bin's pair list (P = 179700
    pairs, 44 chunks of 4096: bins straddle chunk edges).  A pair dropped or doubled by the scatter moves an entry by 1."""
    dev, points = device(N, N)
    with dev:
        check_pair_stage(dev, N, points)
    X, bounds = vl.lattice(N)
    v = gm.VariogramFourthRoot(X, np.eye(N)[:2], bounds, backend="hip")
    np.testing.assert_array_equal(v.bin_locations[1:], np.arange(1., N))          # k (N - k) / (N - k): exact
    v.close()


def test_pair_stage_sums_against_fsum(smooth):
    """dij_sum of smooth curves at the edge bins against math.fsum of numpy's sqrt|z_i - z_j| (sqrt is correctly rounded on both
    sides, so the terms are equal).  A term passes ceil(m / 256) - 1 additions of its lane's chain and the 8 levels of block_sum's
    tree, each with relative error 2^-53, and fsum rounds once: (ceil(m / 256) + 8) 2^-53 sum|term|."""
    v, z = smooth
    for k in EDGE:
        i = np.arange(k, N)
        m = N - k
        for c in range(5):
            terms = np.sqrt(np.abs(z[c, i] - z[c, i - k]))
            want, bound = math.fsum(terms), (-(-m // 256) + 8) * 2.0 ** -53 * math.fsum(terms)
            got = v._dev.dij_sum[k, c]
            print(f"bin {k} curve {c}: |dij_sum - fsum| = {abs(got - want):.2e} (bound {bound:.2e})")
            assert abs(got - want) <= bound, (k, c, got, want)


# ---- cov tiles -------------------------------------------------------------------------------------------------------------------
TILE_REQUESTS = (vl.DIAG + [r for a, b in vl.OFF for r in ((a, b), (b, a))] + [(0, 87), (87, 0), (0, 0)])


def test_cov_tiles_against_the_truth(smooth, golden):
    """Bins of 513, 512, 511, 257, 256, 255, 2 and 1 pairs (tiles of kinds 0, 1 and 2, one-pair tiles present and absent) with
    nc = 5 (a padded last curve group), all requests in one call.  By construction: (a, b) and (b, a) give the same bits (the host
    puts the larger bin on the lanes), a request alone gives the bits of its row in the batch (a request's tile partials and their
    order do not depend on its neighbours), and an empty bin gives exactly 0."""
    v, _ = smooth
    gt = vl.model_gt(N, 5)
    b1, b2 = np.array(TILE_REQUESTS).T
    got = v._dev.cov_sums(gt, VF, CF, b1, b2)
    check_against_truth(got, golden["tiles"], TILE_REQUESTS, label="tiles")
    row = {r: got[n] for n, r in enumerate(TILE_REQUESTS)}
    for a, b in vl.OFF:
        np.testing.assert_array_equal(row[(a, b)], row[(b, a)])
    for r in ((0, 87), (87, 0), (0, 0)):
        np.testing.assert_array_equal(row[r], np.zeros(5))
    for a, b in TILE_REQUESTS:
        np.testing.assert_array_equal(v._dev.cov_sums(gt, VF, CF, [a], [b])[0], row[(a, b)], err_msg=f"alone {(a, b)}")
    # compute(): every bin's diagonal request in one call (the tiles of all 600 requests sorted by work together); its sums are
    # _cov_sums(labels, labels), and on the fourth-root scale its bands are gamma_star_mean -+ sqrt(sum / m^2)
    kept = v.gamma_tilde
    try:
        v.gamma_tilde = gt
        labels = v.bin_labels.astype(np.int32)
        sums = v._cov_sums(labels, labels)
        gam, lo, up = v.compute(rt_scale=True)
    finally:
        v.gamma_tilde = kept
    np.testing.assert_array_equal(sums[0], np.zeros(5))
    for k in EDGE:
        np.testing.assert_array_equal(sums[k], row[(k, k)], err_msg=f"all bins in one call, bin {k}")
        sd = np.sqrt(row[(k, k)] / float((N - k) * (N - k)))
        np.testing.assert_array_equal(lo[k], v.gamma_star_mean[k] - sd)
        np.testing.assert_array_equal(up[k], v.gamma_star_mean[k] + sd)


# ---- curve groups ----------------------------------------------------------------------------------------------------------------
def test_curve_groups(golden):
    """nc = 1, 2, 3 run k_cov<1>, <2>, <3> with one full group; nc = 4 and 8 have full groups of 4; nc = 5, 7 and 9 a padded last
    group (gam, den, sq and slab are indexed by ncp, out by nc).  The curves differ (ell_c = 3 .. 900), so a column or group
    mix-up misses the truth.  By construction only this identity holds and is asserted: for nc >= 4 every call runs k_cov<4> and
    curve c sits at position c % 4 of group c // 4 whatever nc is, so its bits equal those of the nc = 9 call.  nc = 1, 2, 3 run
    other instantiations of the kernel (the compiler may contract differently), so they are checked against the truth only; the
    identity with single-curve calls at equal CG has no instance beyond nc = 1 itself (CG = 1 only there)."""
    reqs = vl.GROUP_REQUESTS
    b1, b2 = np.array(reqs).T
    out = {}
    for nc in (1, 2, 3, 4, 5, 7, 8, 9):
        dev, _ = device(N, nc)
        with dev:
            out[nc] = dev.cov_sums(vl.model_gt(N, nc), VF, CF, b1, b2)
        assert out[nc].shape == (3, nc)
        check_against_truth(out[nc], golden["groups"], reqs, nc=nc, label=f"groups nc={nc}")
    for nc in (4, 5, 7, 8):
        np.testing.assert_array_equal(out[nc], out[9][:, :nc], err_msg=f"nc={nc}")


# ---- request-list cache ----------------------------------------------------------------------------------------------------------
def test_request_list_cache(golden):
    """The tile list, order and tstart stay on the device while the request list repeats; gamma~, den and sq must not."""
    A, B = vl.CACHE_A, vl.CACHE_B
    gt, gt2 = vl.model_gt(N, 2), vl.model_gt(N, 2, variant=1)
    dev, _ = device(N, 2)
    with dev:
        def call(g, reqs):
            return dev.cov_sums(g, VF, CF, *np.array(reqs).T)
        first = call(gt, A)
        check_against_truth(first, golden["tiles"], A, nc=2, label="cache A")
        np.testing.assert_array_equal(call(gt, A), first)
        second = call(gt2, A)
        check_against_truth(second, golden["cache_second_gamma"], A, label="cache A, second gamma~")
        for a, b in A:                                                  # the two truths are far apart: the second call cannot pass on the first's sums
            gap = np.abs(golden["cache_second_gamma"].row(a, b).sum - golden["tiles"].row(a, b).sum[:2])
            assert np.all(gap > 100 * golden["tiles"].atol(a, b)[:2])
        check_against_truth(call(gt, B), golden["tiles"], B, nc=2, label="cache B")
        np.testing.assert_array_equal(call(gt, A), first)


# ---- LDS thresholds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins,nc", [((4097, 4098), 1), ((1536, 1537), 4), ((6144, 6145), 1)],
                         ids=["bounds_4096_4097", "gamma_lds_1536x4_1537x4", "gamma_lds_6144_6145"])
def test_lds_thresholds(golden, nbins, nc):
    """N = 120 with the bounds padded by repeats of 1e6 (empty bins; nbin = bounds + 1): bounds searched in LDS up to 4096 of them
    (nbin = 4097) and in global memory above; gamma~ in LDS while nbin CG <= 6144 (nbin = 1536 | 1537 with CG = 4: 6144 | 6148
    entries; nbin = 6144 | 6145 with CG = 1).  Either side of a threshold runs the same arithmetic on the same values, so the cov
    sums are bit-identical."""
    n = 120
    points = [0, 59, 60, 119][:nc] if nc > 1 else [59]
    reqs = vl.LDS_REQUESTS + [(b, a) for a, b in vl.LDS_REQUESTS if a != b]
    b1, b2 = np.array(reqs).T
    got = []
    for nbin in nbins:
        dev, _ = device(n, nc, nbin - 1, points)
        with dev:
            assert len(dev.counts) == nbin
            check_pair_stage(dev, n, points)
            got.append(dev.cov_sums(vl.model_gt(nbin, nc), VF, CF, b1, b2))
        check_against_truth(got[-1], golden["lds"], reqs, nc=nc, label=f"lds nbin={nbin} nc={nc}")
    np.testing.assert_array_equal(got[0], got[1])


# ---- the chunk cap ---------------------------------------------------------------------------------------------------------------
def test_chunk_cap(golden):
    """N = 2100 with 32767 bins: P = 2203950 pairs ask for 539 chunks of 4096, max_chunks = 2^24 / 32767 = 512 caps them (chunks of
    4352 pairs); also above both LDS thresholds."""
    n, nb = 2100, 32766
    assert -(-(n * (n - 1) // 2) // 4096) == 539 and (1 << 24) // (nb + 1) == 512
    points = [0, 1049, 2099]
    reqs = vl.CAP_REQUESTS + [(1844, 2098)]
    dev, _ = device(n, 3, nb, points)
    with dev:
        check_pair_stage(dev, n, points)
        got = dev.cov_sums(vl.model_gt(nb + 1, 3), VF, CF, *np.array(reqs).T)
    check_against_truth(got, golden["cap"], reqs, label="cap")
    np.testing.assert_array_equal(got[1], got[2])


# ---- distances -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [7, 8, 15, 16, 64])
def test_bins_match_numpy_on_the_bounds_at_the_accumulator_edges(d):
    """bounds = every distinct distance numpy computes, at d = 7 (the last sequential sum), 8 (eight accumulators, no loop, no
    tail), 15 (tail of 7), 16 (one full loop, no tail) and 64 (the maximum): a distance one ulp off changes its bin."""
    n = 60
    X = np.round(np.random.RandomState(100 + d).uniform(0, 4, (n, d)), 1)
    ti, tj = np.tril_indices(n, -1)
    h = np.linalg.norm(X[:, None, :] - X, axis=-1)[ti, tj]
    bounds = np.unique(h)[:32000]
    assert len(bounds) > 1000
    with DeviceVariogram(0, X, np.zeros((1, n)), bounds) as dev:
        np.testing.assert_array_equal(dev.counts, np.bincount(np.digitize(h, bounds), minlength=len(bounds) + 1))
