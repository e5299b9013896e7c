"""Shared cases of the blocked route of the Toeplitz path, ``method="blocked"`` (test_toeplitz_blocked_cpu.py on backend='cpu', where the
keyword selects nothing; test_gpu_toeplitz_blocked.py on 'hip'): DESIGN.md section 23.

Where the panel route exists (n <= 8192) the blocked route is held to it bit for bit: every element of the generator goes through the
same IEEE operations in the same order, and the kernels that consume the panel are the same.  Beyond, the yardsticks are closed forms
(ARFIMA's sum_log_diag, the Kac-Murdock-Szego G), one mpmath golden at n = 8193 and the identity case, each under a bound that comes
from toeplitz_cases or from the panel route's own distance at n = 8192.  B (the panel width) and R (the rows a tile owns) are asked of
the library when a test runs, not when it is collected.  Every check returns what it measured."""
import functools
import json
import os

import numpy as np

import gsum_amd as gm
import toeplitz_cases as tc
import toeplitz_grad_cases as gc
import toeplitz_panel_cases as pn
import toeplitz_post_cases as pc
from toeplitz_cases import EPS, FLOOR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toeplitz_blocked.json")
LIMIT = 8192                                         # gsum_toep_max_n(): where the column and panel routes end
PANEL_BUDGET = pn.PANEL_BUDGET
COLUMN_COUNTS = (1, 17)
WIDE = 257


def width():
    return gm.toeplitz_panel_width()


def tile_rows():
    from gsum_amd import _toep_lib
    return _toep_lib.blocked_tile_rows()


# label -> (multiple of B, multiple of R, offset): one step to three, around one panel, around one tile's own rows, around the first
# row whose halo is whole (R + B), two tiles with a partial third, and the size classes of sum_log_diag's order up to the limit.
_EDGES = {"1": (0, 0, 1), "2": (0, 0, 2), "3": (0, 0, 3), "B-1": (1, 0, -1), "B": (1, 0, 0), "B+1": (1, 0, 1), "2B+1": (2, 0, 1),
          "R-1": (0, 1, -1), "R": (0, 1, 0), "R+1": (0, 1, 1), "R+B-1": (1, 1, -1), "R+B": (1, 1, 0), "R+B+1": (1, 1, 1),
          "2R+17": (0, 2, 17), "513": (0, 0, 513), "2049": (0, 0, 2049), "4097": (0, 0, 4097), "8191": (0, 0, 8191), "8192": (0, 0, 8192)}
EDGE_SIZES = tuple(_EDGES)
# (first column position, label): beyond the limit
_BEYOND = {"8193": (0, 8193), "8192+R+1": (1, 8193), "16385": (0, 16385)}
BEYOND_SIZES = tuple(_BEYOND)


def edge_size(label):
    b, r, off = _EDGES[label]
    return b * width() + r * tile_rows() + off


def beyond_size(label):
    r, off = _BEYOND[label]
    return r * tile_rows() + off


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def check_equal_to_panel(backend, n, ncols):
    """(1): G, sum_log_diag and info of ``method="blocked"`` are those of ``method="panel"`` bit for bit on the two ARFIMA columns."""
    t = pn.arfima_columns(n)
    n_sets, cols = pn.split(ncols)
    Z = tc.rhs_columns(n, ncols, seed=ncols)
    blk = gm.toeplitz_gram(t, Z, n_sets, backend=backend, method="blocked")
    pan = gm.toeplitz_gram(t, Z, n_sets, backend=backend, method="panel")
    assert blk[0].shape == (2, n_sets, cols, cols) and not blk[2].any(), blk[2]
    assert np.array_equal(blk[2], pan[2]) and np.array_equal(blk[1], pan[1]), (n, ncols, blk[1], pan[1])
    assert np.array_equal(blk[0], pan[0]), (n, ncols, float(np.max(np.abs(blk[0] - pan[0]))))
    return dict(sum_log_diag=[float(s) for s in blk[1]])


def check_predict_equal_to_panel(backend, n):
    """(1): quad, cross, cov, G, sum_log_diag and info of ``toeplitz_predict`` on the two routes, bit for bit."""
    t = tc.arfima_column(n, 0.4)
    K, Z = tc.rhs_columns(n, 37, seed=2), tc.rhs_columns(n, 3)
    blk = gm.toeplitz_predict(t, K, Z, want_cov=True, backend=backend, method="blocked")
    pan = gm.toeplitz_predict(t, K, Z, want_cov=True, backend=backend, method="panel")
    assert blk.info == 0 and pan.info == 0 and blk.sum_log_diag == pan.sum_log_diag
    for name in ("quad", "cross", "cov", "G"):
        assert np.array_equal(getattr(blk, name), getattr(pan, name)), (n, name)
    assert np.array_equal(blk.cov, blk.cov.T)
    none = gm.toeplitz_predict(t, K, None, backend=backend, method="blocked")
    assert none.cov is None and none.cross.shape == (37, 0) and np.array_equal(none.quad, blk.quad)
    return float(blk.sum_log_diag)


def check_ill_equal_to_panel(backend, name):
    """(1): the ill-conditioned goldens, whose reflection coefficients come close to 1, where a lost low word moves a pivot."""
    t, Z, Gt, st, _, _ = tc._ill_yardsticks(name)
    blk = gm.toeplitz_gram(t, Z, backend=backend, method="blocked")
    pan = gm.toeplitz_gram(t, Z, backend=backend, method="panel")
    assert blk[2] == 0 and pan[2] == 0
    assert blk[1] == pan[1], (name, blk[1], pan[1])
    assert np.array_equal(blk[0], pan[0]), name
    return tc.distances(blk[0][0], blk[1], Gt, st)


# ---- beyond the limit -------------------------------------------------------------------------------------------------------------------

def check_sum_log_diag(backend, n):
    """(2): sum_log_diag against ARFIMA's closed form within 4 * 64 * 2^-53 relative to max(1, |truth|): the ceiling of
    toeplitz_cases._rule (the cpu backend, which sets the factor below the ceiling, is too slow here)."""
    t = pn.arfima_columns(n)
    G, sld, info = gm.toeplitz_gram(t, tc.rhs_columns(n, 2), 1, backend=backend, method="blocked")
    assert not info.any() and np.isfinite(G).all() and np.array_equal(G, G.transpose(0, 1, 3, 2))
    truth = [tc.arfima_sum_log_diag(n, d) for d in tc.DS]
    d = [abs(sld[i] - truth[i]) / max(1.0, abs(truth[i])) for i in range(2)]
    print(f"toeplitz blocked sum_log_diag {backend} n={n}: " + ", ".join(f"{x / EPS:.2f} eps" for x in d))
    assert max(d) <= 4 * FLOOR, (n, d)
    return dict(sld_eps=[x / EPS for x in d])


KMS_CPU_LIMIT = 8192 + 1024                          # the largest n at which the cpu backend sets the closed form's bound inside a test


def check_kms(backend, n):
    """(2): G and sum_log_diag on the Kac-Murdock-Szego columns (rho = 0.5, -0.25: exact in fp64) against the closed form, under
    toeplitz_cases.check_closed_form's bound: the floor times the cpu backend's own factor over it, between 1 and 4
    (``toeplitz_cases.kms_distances("cpu", n)``, computed once per n).  The cpu backend's two columns take 3.0 s at n = 8193 and
    4.0 s at 8192 + R + 1; at n = 16385 they take 11.6 s, too long for a test that runs with every later change.  There the bound is
    one floor, the least that rule can give whatever the cpu backend measures, so it asks no less than the rule and needs no cpu
    run (the cpu backend, run once by hand, sits at 28.8 and 11.6 * 2^-53 there: the rule gives the same floor)."""
    t, Z, truth = tc._kms_inputs(n, 4, 1, 2)
    G, sld, info = gm.toeplitz_gram(t, Z, 1, backend=backend, method="blocked")
    assert not info.any() and np.array_equal(G, G.transpose(0, 1, 3, 2))
    d = [tc.distances(G[i], sld[i], *truth[i]) for i in range(2)]
    got = max(x[0] for x in d), max(x[1] for x in d)
    cpu = tc.kms_distances("cpu", n) if n <= KMS_CPU_LIMIT else None
    bounds = tuple(tc._rule(x) for x in cpu) if cpu else (FLOOR, FLOOR)
    print(f"toeplitz blocked closed form {backend} n={n}: G {got[0] / EPS:.2f} eps, sum_log_diag {got[1] / EPS:.2f} eps" +
          (f" (cpu {cpu[0] / EPS:.2f}, {cpu[1] / EPS:.2f})" if cpu else " (cpu not run: one floor)"))
    assert got[0] <= bounds[0] and got[1] <= bounds[1], (n, got, bounds)
    return dict(G_eps=got[0] / EPS, sld_eps=got[1] / EPS, bound_G_eps=bounds[0] / EPS, bound_sld_eps=bounds[1] / EPS)


def blocked_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _golden_distance(G, Gt):
    return max(float(np.max(np.abs(G[i] - Gt[i])) / np.max(np.abs(Gt[i]))) for i in range(2))


def check_arfima_golden(backend):
    """(2): G of the ARFIMA columns at n = 8193 against the committed mpmath golden, under ``_rule`` of the panel route's own distance
    from the n = 8192 golden: the floor times the panel route's factor over it, at most 4 floors."""
    gold = {c["d"]: c for c in blocked_golden()["arfima"]}
    n = gold[tc.DS[0]]["n"]
    assert n == LIMIT + 1
    t, Z = pn.arfima_columns(n), tc.rhs_columns(n, 4)
    G, sld, info = gm.toeplitz_gram(t, Z, 1, backend=backend, method="blocked")
    assert not info.any()
    d_g = _golden_distance(G[:, 0], [np.array(gold[d]["G"]) for d in tc.DS])
    d_s = max(abs(sld[i] - gold[d]["sum_log_diag"]) / max(1.0, abs(gold[d]["sum_log_diag"])) for i, d in enumerate(tc.DS))
    t8, Z8, _, G8 = tc._arfima_inputs(LIMIT)
    Gp, _, ip = gm.toeplitz_gram(t8, Z8, 1, backend=backend, method="panel")
    assert not ip.any()
    p_g = _golden_distance(Gp[:, 0], G8)
    print(f"toeplitz blocked arfima golden {backend} n={n}: G {d_g / EPS:.2f} eps (panel at {LIMIT}: {p_g / EPS:.2f}), sum_log_diag {d_s / EPS:.2f} eps")
    assert d_g <= tc._rule(p_g), (d_g, p_g)
    assert d_s <= 4 * FLOOR, d_s
    return dict(G_eps=d_g / EPS, panel_8192_G_eps=p_g / EPS, sld_eps=d_s / EPS)


@functools.lru_cache(maxsize=None)
def identity_pieces(backend, n, method):
    """The distances (quad, cross, cov) of the identity case on ARFIMA(0.4): K = the columns idx of T gives quad = t_0, cross = Z[idx]
    and cov = T[idx, idx].  idx: both ends, the rows around the first panel, the first tile and the limit, and 16 spread evenly."""
    B, R = width(), tile_rows()
    t, Z = tc.arfima_column(n, 0.4), tc.rhs_columns(n, 4)
    idx = np.array(sorted({i for i in [0, 1, B - 1, B, R - 1, R, R + B, n // 2, LIMIT - 1, LIMIT, n - 2, n - 1] + [(j * (n - 1)) // 17 for j in range(1, 17)]
                           if 0 <= i < n}))
    K = t[np.abs(np.arange(n)[:, None] - idx[None, :])]
    r = gm.toeplitz_predict(t, K, Z, want_cov=True, backend=backend, method=method)
    assert r.info == 0 and np.array_equal(r.cov, r.cov.T)
    return pc.piece_distances((r.quad, r.cross, r.cov), (np.full(len(idx), t[0]), Z[idx], K[idx]))


def check_identity(backend, n):
    """(2): each piece of the identity case within 4 x max(the panel route's distance on the same case at n = 8192, 64 * 2^-53): 4 is the
    project's factor between two implementations, and ARFIMA's conditioning grows by less than 2 from 8192 to 16385."""
    got, pan = identity_pieces(backend, n, "blocked"), identity_pieces(backend, LIMIT, "panel")
    print(f"toeplitz blocked identity {backend} n={n}: " + ", ".join(f"{pc.PIECES[k]} {got[k] / EPS:.2f} eps (panel at {LIMIT}: {pan[k] / EPS:.2f})" for k in range(3)))
    for k in range(3):
        assert got[k] <= 4 * max(pan[k], FLOOR), (n, pc.PIECES[k], got, pan)
    return {**{p: g / EPS for p, g in zip(pc.PIECES, got)}, **{"panel_8192_" + p: g / EPS for p, g in zip(pc.PIECES, pan)}}


# ---- independence -----------------------------------------------------------------------------------------------------------------------

def check_independence(backend, n):
    """(3): a (first column, column) result is bitwise unchanged under permuting the columns, halving them, padding with 300 others and
    m = 1 against 3; cov is bitwise symmetric."""
    rng = np.random.RandomState(7)
    t1 = tc.arfima_column(n, 0.4)
    q = 21
    K, Z = rng.randn(n, q), rng.randn(n, 3)

    def predict(K_, **kw):
        return gm.toeplitz_predict(t1, K_, Z, backend=backend, method="blocked", **kw)

    full = predict(K, want_cov=True)
    assert full.info == 0 and np.array_equal(full.cov, full.cov.T)
    perm = rng.permutation(q)
    assert pc._pieces_equal(predict(K[:, perm], want_cov=True), full, perm)
    half = np.arange(0, q, 2)
    assert pc._pieces_equal(predict(K[:, half], want_cov=True), full, half)
    more = predict(np.concatenate([rng.randn(n, 150), K, rng.randn(n, 150)], axis=1), want_cov=True)
    assert pc._pieces_equal(full, more, np.arange(150, 150 + q))
    G1, s1, i1 = gm.toeplitz_gram(t1, Z, 1, backend=backend, method="blocked")
    assert i1 == 0 and np.array_equal(G1[0], full.G) and s1 == full.sum_log_diag
    G3, s3, i3 = gm.toeplitz_gram(np.stack([tc.arfima_column(n, -0.3), t1, tc.arfima_column(n, 0.25)]), Z, 1, backend=backend, method="blocked")
    assert not i3.any() and np.array_equal(G3[1], G1) and s3[1] == s1                    # m = 1 against m = 3
    return float(s1)


def blocked_bytes(n, ncols):
    """The library's arithmetic (gsum_toep.hip: blocked_bytes): the solved columns with their fp32 words, one panel, the two generator
    states, the panel's coefficients and the diagonal of L."""
    return n * ncols * 12 + n * width() * 12 + (2 * 4 * n + 4 * width() + n) * 8


def first_columns_per_launch(n, ncols, m, budget=PANEL_BUDGET):
    return max(1, min(m, 65535, budget // blocked_bytes(n, ncols)))


def chunked_shape(n):
    """(c, n_sets, m) whose three first columns do not fit the budget together at order n, while two do."""
    c, m = 16, 3
    return c, ((PANEL_BUDGET // m) - (n * width() * 12 + (9 * n + 4 * width()) * 8)) // (n * 12 * c) + 1, m


def check_chunk_loop(backend, n):
    """(3): three first columns that go through as two and one.  For each, G of the first, middle and last set and sum_log_diag are
    bitwise those of a call with that first column and those three sets alone.  Device only."""
    c, n_sets, m = chunked_shape(n)
    assert first_columns_per_launch(n, n_sets * c, m) == 2
    ts = np.stack([tc.arfima_column(n, d) for d in (0.4, -0.3, 0.25)])
    Z = np.asfortranarray(np.random.RandomState(11).standard_normal((n_sets * c, n)).T)
    G, sld, info = gm.toeplitz_gram(ts, Z, n_sets, backend=backend, method="blocked")
    assert not info.any()
    pick = [0, n_sets // 2, n_sets - 1]
    Z3 = np.concatenate([Z[:, s * c:(s + 1) * c] for s in pick], axis=1)
    for i in range(m):
        Gs, ss, is_ = gm.toeplitz_gram(ts[i], Z3, 3, backend=backend, method="blocked")
        assert is_ == 0 and np.array_equal(G[i][pick], Gs) and sld[i] == ss, i
    return [int(x) for x in info]


# ---- failures ---------------------------------------------------------------------------------------------------------------------------

def failure_positions(n):
    """The edited entries p (the recursion fails in step p - 1, info = p + 1): the first steps, around the first panel's end, around
    the first tile's end, where the second tile's halo is whole, around the limit of the other routes, and the last two."""
    B, R = width(), tile_rows()
    ps = [1, 2, B - 1, B, B + 1, R - 1, R, R + 1, R + B, LIMIT - 1, LIMIT, LIMIT + 1, n - 2, n - 1]
    return sorted({p for p in ps if 1 <= p <= n - 1}), min(n - 1, R + B + 3)


def check_late_failures(backend, n, d=0.25):
    """(4): t_p + 1.5 E_{p-1} of an ARFIMA column fails at step p + 1 exactly; a NaN in t at its step.  All failing first columns in
    one call between healthy ones, which come out bit for bit as they do alone."""
    good = tc.arfima_column(n, d)
    En = tc.arfima_energies(n, d)
    ps, p_nan = failure_positions(n)
    bad = []
    for p in ps:
        t = good.copy()
        t[p] += 1.5 * float(En[p - 1])
        bad.append(t)
    t = good.copy()
    t[p_nan] = np.nan
    bad.append(t)
    want = [p + 1 for p in ps] + [p_nan + 1]
    half = len(bad) // 2
    other = tc.arfima_column(n, -0.3)
    Z = tc.rhs_columns(n, 18)
    G0, s0, i0 = gm.toeplitz_gram(good, Z, 2, backend=backend, method="blocked")
    G1, s1, i1 = gm.toeplitz_gram(other, Z, 2, backend=backend, method="blocked")
    assert i0 == 0 and i1 == 0
    G, sld, info = gm.toeplitz_gram(np.stack([other] + bad[:half] + [good] + bad[half:] + [other]), Z, 2, backend=backend, method="blocked")
    assert list(info) == [0] + want[:half] + [0] + want[half:] + [0], (n, list(info))
    healthy = [0, half + 1, len(info) - 1]
    rest = np.setdiff1d(np.arange(len(info)), healthy)
    assert np.isnan(sld[rest]).all() and np.isnan(G[rest]).all()
    assert np.array_equal(G[half + 1], G0) and sld[half + 1] == s0
    for i in (0, len(info) - 1):
        assert np.array_equal(G[i], G1) and sld[i] == s1
    r = gm.toeplitz_predict(bad[1], tc.rhs_columns(n, 5, seed=2), Z[:, :2], want_cov=True, backend=backend, method="blocked")
    assert r.info == ps[1] + 1 and all(np.isnan(a).all() for a in (r.quad, r.cross, r.cov, r.G)) and np.isnan(r.sum_log_diag)
    return [int(x) for x in info]


# ---- the other routes -------------------------------------------------------------------------------------------------------------------

def check_other_routes_undisturbed():
    """(5), device only: the column and panel routes' results on toeplitz_cases.SHAPES are bit-equal before and after blocked calls on
    the same handle, their four clocks are not charged by them, and the blocked clock's eight phases all are."""
    from gsum_amd import _toep_lib
    h = _toep_lib.default_handle(0)

    def earlier():
        out = []
        for ns, c, n_sets, m in tc.SHAPES:
            ts, Zs, _ = tc._kms_inputs(ns, c, n_sets, m)
            for method in ("columns", "panel"):
                out += list(gm.toeplitz_gram(ts, Zs, n_sets, method=method))
                out += list(gm.toeplitz_predict(ts[0], Zs[:, :c], Zs[:, :1], want_cov=True, method=method))[:4]
        return out

    before = earlier()
    clocks = h.times(), h.grad_times(), h.post_times(), h.panel_times()
    h.blocked_times(reset=True)
    n = tile_rows() + width() + 17
    rng = np.random.RandomState(5)
    t1 = tc.arfima_column(n, 0.4)
    gm.toeplitz_gram(t1, rng.randn(n, 33), 3, method="blocked")
    gm.toeplitz_predict(t1, rng.randn(n, 33), rng.randn(n, 2), want_cov=True, method="blocked")
    assert (h.times(), h.grad_times(), h.post_times(), h.panel_times()) == clocks
    ms = h.blocked_times()
    assert tuple(ms) == _toep_lib.BLOCKED_PHASES and all(v > 0 for v in ms.values()), ms
    assert _same(earlier(), before)
    return ms


# ---- the model layer --------------------------------------------------------------------------------------------------------------------

def check_surface(backend, n):
    """(6): log_marginal_likelihood_grid(structure="toeplitz", toeplitz_method="blocked") is the panel route's surface bit for bit."""
    gp, thetas, ratios = pn.surface_process(backend, n)
    want = gp.log_marginal_likelihood_grid(thetas, ratios, structure="toeplitz", toeplitz_method="panel")
    got = gp.log_marginal_likelihood_grid(thetas, ratios, structure="toeplitz", toeplitz_method="blocked")
    assert got.shape == (8, 8) and np.isfinite(got).all() and np.array_equal(got, want)
    return float(np.max(got))


def check_model(backend, name, n):
    """(6): wherever ``"panel"`` is accepted ``"blocked"`` is, with the panel route's values bit for bit: log_marginal_likelihood and
    _batch, a fit with dense_factor=False (whose final toeplitz_gram takes the blocked route, and no other fit's does), predict."""
    import pytest
    from gsum_amd import toeplitz as tz
    cls, kw = gc.model_class(name), dict(gc.MODEL_CLASSES)[name]
    X, y = gc.model_xy(n)
    seen = []
    real = tz.toeplitz_gram

    def spy(*a, **k):
        seen.append(k.get("method", "columns"))
        return real(*a, **k)

    tz.toeplitz_gram = spy
    try:
        gp = gc.model_process(cls, backend, optimizer=None, **kw).fit(X, y, structure="toeplitz", dense_factor=False, toeplitz_method="blocked")
        assert seen == ["blocked"], seen
        pan = gc.model_process(cls, backend, optimizer=None, **kw).fit(X, y, structure="toeplitz", dense_factor=False, toeplitz_method="panel")
        assert seen == ["blocked", "columns"], seen
    finally:
        tz.toeplitz_gram = real
    assert gp._toeplitz_method == "blocked" and gp.structure_ == "toeplitz" and gp.corr_L_ is None
    Xs = pc.new_points(X)
    worst = 0.0
    for call in pc.PREDICT_CALLS:
        for o, w in zip(pc._as_tuple(gp.predict(Xs, **call)), pc._as_tuple(pan.predict(Xs, **call))):
            assert o.shape == w.shape and np.isfinite(o).all()
            worst = max(worst, float(np.max(np.abs(o - w)) / np.max(np.abs(w))))
            assert np.max(np.abs(o - w)) <= 1e-9 * np.max(np.abs(w)), call         # the rule of toeplitz_post_cases.check_model between routes
    assert np.array_equal(pan.predict(Xs, toeplitz_method="blocked"), pan.predict(Xs))
    thetas = list(gc.MODEL_THETAS)
    want = gp.log_marginal_likelihood_batch(thetas, structure="toeplitz", toeplitz_method="panel")
    got = gp.log_marginal_likelihood_batch(thetas, structure="toeplitz", toeplitz_method="blocked")
    assert np.array_equal(got, want)
    assert got[1] == gp.log_marginal_likelihood(thetas[1], structure="toeplitz", toeplitz_method="blocked")
    with pytest.raises(ValueError, match="toeplitz_method"):
        gp.predict(Xs, toeplitz_method="Blocked")
    return worst


def check_fit_beyond_the_limit(backend, n=LIMIT + 1, q=5):
    """(6): fit(optimizer=None, structure="toeplitz", dense_factor=False, toeplitz_method="blocked") and predict(return_std=True) at
    n = 8193 run, and so does the same on the grid's first 8192 points; finiteness and shapes, no tolerance: the extra point moves
    the posterior by what it knows."""
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    X = np.linspace(0, 1, n)[:, None]
    y = np.random.RandomState(1).randn(n, 2)
    Xs = np.linspace(0.05, 0.95, q)[:, None] + 0.37 / n
    out = []
    for k in (n, LIMIT):
        gp = gm.ConjugateGaussianProcess(kernel=Matern(0.2, nu=0.5) + WhiteKernel(1e-6, noise_level_bounds="fixed"), optimizer=None, backend=backend,
                                         center=0.1, disp=1.5, df=2, scale=0.7)
        gp.fit(X[:k], y[:k], structure="toeplitz", dense_factor=False, toeplitz_method="blocked")
        assert gp.structure_ == "toeplitz" and gp._toeplitz_method == "blocked"
        mean, std = gp.predict(Xs, return_std=True)
        assert mean.shape == (q, 2) and std.shape == (q,) and np.isfinite(mean).all() and np.isfinite(std).all() and (std > 0).all()
        out.append((mean, std))
    return float(np.max(np.abs(out[0][0] - out[1][0]))), float(np.max(np.abs(out[0][1] - out[1][1])))
