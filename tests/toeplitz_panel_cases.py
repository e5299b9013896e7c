"""Shared cases of the panel route of the Toeplitz path, ``method="panel"`` (test_toeplitz_panel_cpu.py on backend='cpu', where the keyword
selects nothing and every check is one of the cpu backend against itself; test_gpu_toeplitz_panel.py on 'hip'): DESIGN.md section 21.

The yardsticks are those of toeplitz_cases.py and toeplitz_post_cases.py, with no new number: against a truth the backend is within
``max(4 x the cpu backend's distance, 64 * 2^-53 of the largest magnitude)`` and, on the mpmath goldens, within numpy's dense fp64
route's distance on the same T; where there is no truth the two routes are held to each other within the sum of their two bounds,
2 * 4 * 64 * 2^-53 of the largest magnitude.  ``sum_log_diag`` and ``info`` come from the same recursion on both routes: bit-equal.
Every check takes the backend and returns what it measured."""
import functools

import numpy as np

import gsum_amd as gm
import toeplitz_cases as tc
import toeplitz_grad_cases as gc
import toeplitz_post_cases as pc
from toeplitz_cases import EPS, FLOOR

BETWEEN_ROUTES = 2 * 4 * FLOOR                       # two implementations of one recursion, each within 4 floors (toeplitz_cases.check_arfima)
CLASS_EDGES = (512, 513, 2048, 2049, 4096, 4097, 8191, 8192)
COLUMN_COUNTS = (1, 15, 16, 17, 33)                  # around one 16-column MFMA tile, and into the third
WIDE = 257                                           # more than four 64-column groups of the trailing update, and a partial tile
PANEL_BUDGET = 1 << 30                               # bytes of first columns in flight (gsum_toep.hip: kPanelBudget)


def width():
    return gm.toeplitz_panel_width()


# One step, two, around one MFMA tile of rows, around one panel and two, and two panels with a partial row tile beyond them.  Written
# in the panel width B, which the library is asked for when a test runs, not when it is collected: label -> (multiple of B, offset).
_EDGES = {"1": (0, 1), "2": (0, 2), "15": (0, 15), "16": (0, 16), "17": (0, 17), "B-1": (1, -1), "B": (1, 0), "B+1": (1, 1),
          "2B-1": (2, -1), "2B": (2, 0), "2B+1": (2, 1), "2B+17": (2, 17)}
EDGE_SIZES = tuple(_EDGES)


def edge_size(label):
    mult, off = _EDGES[label]
    return mult * width() + off


def split(ncols):
    """(n_sets, cols) with cols <= 16 of a column count: as few sets as divide it."""
    cols = max(c for c in range(1, 17) if ncols % c == 0)
    return ncols // cols, cols


def arfima_columns(n):
    """(2, n): d alternating 0.4 / -0.3, every step of the recursion rotates."""
    return np.stack([tc.arfima_column(n, d) for d in tc.DS])


def check_edges(backend, n, ncols):
    """Panel and tile edges on ARFIMA columns: sum_log_diag against the closed form under the rule of toeplitz_cases (the floor times
    the cpu backend's factor over it, at most 4); G against the column route within the sum of the two bounds; sum_log_diag and info
    bit-equal to the column route's; G exactly symmetric."""
    t = arfima_columns(n)
    n_sets, cols = split(ncols)
    Z = tc.rhs_columns(n, ncols, seed=ncols)
    Gp, sp, ip = gm.toeplitz_gram(t, Z, n_sets, backend=backend, method="panel")
    Gc, sc, ic = gm.toeplitz_gram(t, Z, n_sets, backend=backend)
    assert Gp.shape == (2, n_sets, cols, cols) and not ip.any(), ip
    assert np.array_equal(ip, ic) and np.array_equal(sp, sc), (n, ncols, sp, sc)
    assert np.array_equal(Gp, Gp.transpose(0, 1, 3, 2))
    truth = [tc.arfima_sum_log_diag(n, d) for d in tc.DS]
    d_s = max(abs(sp[i] - truth[i]) / max(1.0, abs(truth[i])) for i in range(2))
    _, s_cpu = tc._arfima_results("cpu", n) if n >= 3 else (None, sp)
    c_s = max(abs(s_cpu[i] - truth[i]) / max(1.0, abs(truth[i])) for i in range(2))
    d_g = float(np.max(np.abs(Gp - Gc)) / np.max(np.abs(Gc)))
    out = dict(sld_eps=d_s / EPS, cpu_sld_eps=c_s / EPS, G_vs_columns_eps=d_g / EPS, bit_equal=bool(np.array_equal(Gp, Gc)))
    print(f"toeplitz panel edges {backend} n={n} ncols={ncols}: " + ", ".join(f"{k} {v}" for k, v in out.items()))
    assert d_s <= tc._rule(c_s), (n, d_s, c_s)
    assert d_g <= BETWEEN_ROUTES, (n, ncols, d_g)
    return out


def check_arfima_golden(backend, n):
    """G of the panel route against the committed mpmath golden of the ARFIMA columns (n = 513, 2049, 4097, 8192), under the rule."""
    t, Z, st, Gt = tc._arfima_inputs(n)
    assert Gt is not None
    G, sld, info = gm.toeplitz_gram(t, Z, 1, backend=backend, method="panel")
    assert not info.any()
    Gc, sc = tc._arfima_results("cpu", n)
    d_g = max(float(np.max(np.abs(G[i, 0] - Gt[i])) / np.max(np.abs(Gt[i]))) for i in range(2))
    c_g = max(float(np.max(np.abs(Gc[i] - Gt[i])) / np.max(np.abs(Gt[i]))) for i in range(2))
    d_s = max(abs(sld[i] - st[i]) / max(1.0, abs(st[i])) for i in range(2))
    c_s = max(abs(sc[i] - st[i]) / max(1.0, abs(st[i])) for i in range(2))
    print(f"toeplitz panel arfima golden {backend} n={n}: G {d_g / EPS:.2f} eps (cpu {c_g / EPS:.2f}), sum_log_diag {d_s / EPS:.2f} eps (cpu {c_s / EPS:.2f})")
    assert d_g <= tc._rule(c_g), (n, d_g, c_g)
    assert d_s <= tc._rule(c_s), (n, d_s, c_s)
    return dict(G_eps=d_g / EPS, cpu_G_eps=c_g / EPS, sld_eps=d_s / EPS)


def check_ill(backend, name):
    """toeplitz_cases.check_ill through the panel route: at most numpy's dense fp64 Cholesky's distance from the mpmath truth on the
    same T (with the floor), and within 4 x the cpu backend's.  Two checks against the column route beside them.  sum_log_diag and
    info are bit-equal: one recursion, and these reflection coefficients come close to 1, where a low word lost between two panels
    moves a pivot (measured: rbf_n2049's sum_log_diag moves by 1.8e-11).  And G is no farther from the truth than 4 x the column
    route's own distance, floor 64 * 2^-53: the column route is the reference the panel route's substitution is copied from, entry
    by entry, so its own error is the measure, and 4 is the yardstick's factor between two implementations of one algorithm.  The
    cpu backend's distance cannot serve here: its substitution has no correction word, so it sits where a panel route that drops
    the word sits or beyond (matern52_n513: column route 3.6e-14, without the word in the trailing update 1.0e-12, cpu 4.9e-9)."""
    t, Z, Gt, st, d_np, d_cpu = tc._ill_yardsticks(name)
    G, sld, info = gm.toeplitz_gram(t, Z, backend=backend, method="panel")
    assert info == 0
    Gc, sc, ic = gm.toeplitz_gram(t, Z, backend=backend)
    assert ic == 0 and sld == sc, (name, sld, sc)
    d, d_col = tc.distances(G[0], sld, Gt, st), tc.distances(Gc[0], sc, Gt, st)
    print(f"toeplitz panel golden {name} {backend}: G {d[0]:.3g} (columns {d_col[0]:.3g}, numpy {d_np[0]:.3g}, cpu {d_cpu[0]:.3g}), "
          f"sum_log_diag {d[1]:.3g}")
    for k in range(2):
        assert d[k] <= max(d_np[k], FLOOR), (name, k, d, d_np)
        assert d[k] <= 4 * max(d_cpu[k], FLOOR), (name, k, d, d_cpu)
    assert d[0] <= 4 * max(d_col[0], FLOOR), (name, d, d_col)
    return d, d_np, d_cpu


def check_offgrid(backend, name):
    """toeplitz_post_cases.check_offgrid through the panel route: quad, cross and cov against the mpmath truth, both bounds."""
    t, K, Z, truth, d_np = pc._offgrid_inputs(name)
    r = gm.toeplitz_predict(t, K, Z, want_cov=True, backend=backend, method="panel")
    assert r.info == 0 and np.array_equal(r.cov, r.cov.T)
    d, d_cpu = pc.piece_distances((r.quad, r.cross, r.cov), truth), pc._offgrid_distances("cpu", name)
    print(f"toeplitz panel off-grid golden {name} {backend}: " +
          ", ".join(f"{pc.PIECES[k]} {d[k]:.3g} (numpy {d_np[k]:.3g}, cpu {d_cpu[k]:.3g})" for k in range(3)))
    if backend == "cpu":                                                # the cpu backend's own yardstick (toeplitz_post_cases.check_offgrid)
        for k in range(3):
            assert d[k] <= 4 * max(d_np[k], FLOOR), (name, pc.PIECES[k], d, d_np)
    else:
        pc._under_golden_bounds(name, pc.PIECES, d, d_np, d_cpu)
    G, sld, info = gm.toeplitz_gram(t, Z, backend=backend, method="panel")
    assert np.array_equal(r.G, G[0]) and r.sum_log_diag == sld          # predict's G is gram's, on this route too
    col = gm.toeplitz_predict(t, K[:, :1], None, backend=backend)
    assert col.info == 0 and r.sum_log_diag == col.sum_log_diag          # ... and the recursion is the column route's
    return d, d_np, d_cpu


def check_identity(backend, n):
    """The identity case of toeplitz_post_cases (K = columns of T: quad = t_0, cross = rows of Z, cov = T[idx, idx]) through the panel
    route, under its yardstick against the cpu backend's own distances."""
    ds, t, _, Z = gc._identity_inputs(n)
    idx = pc.identity_indices(n)
    worst = [0.0, 0.0, 0.0]
    for ti in t:
        K = ti[np.abs(np.arange(n)[:, None] - idx[None, :])]
        r = gm.toeplitz_predict(ti, K, Z, want_cov=True, backend=backend, method="panel")
        assert r.info == 0 and np.array_equal(r.cov, r.cov.T)
        d = pc.piece_distances((r.quad, r.cross, r.cov), (np.full(len(idx), ti[0]), Z[idx], K[idx]))
        worst = [max(a, b) for a, b in zip(worst, d)]
    cpu = pc.identity_distances("cpu", n)
    print(f"toeplitz panel identity {backend} n={n}: " + ", ".join(f"{pc.PIECES[k]} {worst[k] / EPS:.2f} eps (cpu {cpu[k] / EPS:.2f})" for k in range(3)))
    for k in range(3):
        assert worst[k] <= pc.yardstick(cpu[k]), (n, pc.PIECES[k], worst, cpu)
    return dict(zip(pc.PIECES, (w / EPS for w in worst)))


# ---- independence -----------------------------------------------------------------------------------------------------------------------

def check_gram_independence(backend):
    """At n = 2 B + 17: the G of a (first column, set) is bitwise reproducible and unchanged under reversing the sets, dropping half
    of them, adding 300 others and m = 1 against m = 3."""
    n = 2 * width() + 17
    rng = np.random.RandomState(3)
    t1 = tc.arfima_column(n, 0.4)
    c = 5
    Zs = rng.randn(80, n, c)

    def flat(sets):
        return sets.transpose(1, 0, 2).reshape(n, -1)

    def gram(t, sets):
        return gm.toeplitz_gram(t, flat(sets), len(sets), backend=backend, method="panel")

    G, s, i = gram(t1, Zs)
    assert i == 0
    G2, s2, _ = gram(t1, Zs)
    assert np.array_equal(G, G2) and s == s2                                          # two runs
    assert np.array_equal(gram(t1, Zs[::-1])[0][::-1], G)                             # the sets reversed
    assert np.array_equal(gram(t1, Zs[::2])[0], G[::2])                               # half of them dropped
    more = np.concatenate([rng.randn(150, n, c), Zs, rng.randn(150, n, c)])
    assert np.array_equal(gram(t1, more)[0][150:230], G)                              # 300 others around them
    assert np.array_equal(gram(t1, Zs[:1])[0], G[:1])                                 # one set alone: a single column tile
    G3, s3, i3 = gram(np.stack([tc.arfima_column(n, -0.3), t1, tc.arfima_column(n, 0.25)]), Zs)
    assert not i3.any() and np.array_equal(G3[1], G) and s3[1] == s                    # m = 1 against m = 3


def first_columns_per_launch(n, ncols, m, budget=PANEL_BUDGET):
    """The library's arithmetic (gsum_toep.hip: panel_bytes): the solved columns with their fp32 words, one panel, the generator state."""
    per = n * ncols * 12 + n * width() * 12 + 4 * 512 * tc.elements_per_thread(n) * 8
    return max(1, min(m, 65535, budget // per))


def chunked_shape():
    """(n, c, n_sets, m) at n = 2 B + 17 whose three first columns do not fit the budget together, while two do."""
    n, c, m = 2 * width() + 17, 16, 3
    return n, c, (PANEL_BUDGET // m) // (n * 12 * c) + 1, m


def check_chunk_loop(backend):
    """A call whose first columns exceed the library's budget of 1 GiB, so that its three first columns go through two and one
    (offsets into t, sum_log_diag, info and G; the buffers reused).  For each, G of the first, middle and last set and sum_log_diag
    are bitwise those of a call with that first column and those three sets alone.  Device only (240 MB of Z)."""
    n, c, n_sets, m = chunked_shape()
    assert first_columns_per_launch(n, n_sets * c, m) == 2
    ts = np.stack([tc.arfima_column(n, d) for d in (0.4, -0.3, 0.25)])
    Z = np.asfortranarray(np.random.RandomState(11).standard_normal((n_sets * c, n)).T)
    G, sld, info = gm.toeplitz_gram(ts, Z, n_sets, backend=backend, method="panel")
    assert not info.any()
    pick = [0, n_sets // 2, n_sets - 1]
    Z3 = np.concatenate([Z[:, s * c:(s + 1) * c] for s in pick], axis=1)
    for i in range(m):
        Gs, ss, is_ = gm.toeplitz_gram(ts[i], Z3, 3, backend=backend, method="panel")
        assert is_ == 0 and np.array_equal(G[i][pick], Gs) and sld[i] == ss, i
    return [int(x) for x in info]


def check_predict_independence(backend):
    """At n = 2 B + 17: quad, cross and cov[a, b] are bitwise unchanged under permuting the new points, dropping half of them, adding
    300 others, the ``chunk`` loop and whether cov is asked for; cov is bitwise symmetric; (2^a K, 2^b Z, 4^j t) moves the results by
    exact powers of two."""
    n = 2 * width() + 17
    rng = np.random.RandomState(7)
    t1 = tc.arfima_column(n, 0.4)
    q = 37
    K, Z = rng.randn(n, q), rng.randn(n, 3)

    def predict(K_, Z_=Z, t=t1, **kw):
        return gm.toeplitz_predict(t, K_, Z_, backend=backend, method="panel", **kw)

    full = predict(K, want_cov=True)
    assert full.info == 0 and np.array_equal(full.cov, full.cov.T)
    assert pc._pieces_equal(predict(K, want_cov=True), full)
    perm = rng.permutation(q)
    assert pc._pieces_equal(predict(K[:, perm], want_cov=True), full, perm)
    half = np.arange(0, q, 2)
    assert pc._pieces_equal(predict(K[:, half], want_cov=True), full, half)
    more = predict(np.concatenate([rng.randn(n, 150), K, rng.randn(n, 150)], axis=1), want_cov=True)
    assert pc._pieces_equal(full, more, np.arange(150, 150 + q))
    chunked = predict(K, chunk=5)
    assert chunked.cov is None and pc._pieces_equal(chunked, full) and np.array_equal(chunked.G, full.G) and chunked.sum_log_diag == full.sum_log_diag
    assert pc._pieces_equal(predict(K), full)
    none = predict(K, None, want_cov=True)
    assert none.cross.shape == (q, 0) and np.array_equal(none.quad, full.quad) and np.array_equal(none.cov, full.cov)
    b = 7
    for a, j in tc.SCALINGS:
        sc = predict(2.0 ** a * K, 2.0 ** b * Z, 4.0 ** j * t1, want_cov=True)
        assert sc.info == 0
        assert np.array_equal(sc.quad, 2.0 ** (2 * a - 2 * j) * full.quad) and np.array_equal(sc.cov, 2.0 ** (2 * a - 2 * j) * full.cov), (a, j)
        assert np.array_equal(sc.cross, 2.0 ** (a + b - 2 * j) * full.cross) and np.array_equal(sc.G, 2.0 ** (2 * b - 2 * j) * full.G), (a, j)
    # against the column route: within the sum of the two bounds; sum_log_diag bit-equal
    col = gm.toeplitz_predict(t1, K, Z, want_cov=True, backend=backend)
    for name in ("quad", "cross", "cov", "G"):
        assert pc.rel(getattr(full, name), getattr(col, name)) <= BETWEEN_ROUTES, name
    assert full.sum_log_diag == col.sum_log_diag
    return bool(pc._pieces_equal(full, col))


def check_column_route_undisturbed():
    """Device only: the column route's results on toeplitz_cases.SHAPES are bit-equal before and after panel calls on the same handle,
    its three clocks are not charged by them, and the panel clock's seven phases all are."""
    from gsum_amd import _toep_lib
    h = _toep_lib.default_handle(0)

    def earlier():
        out = []
        for ns, c, n_sets, m in tc.SHAPES:
            ts, Zs, _ = tc._kms_inputs(ns, c, n_sets, m)
            out += list(gm.toeplitz_gram(ts, Zs, n_sets))
            out += list(gm.toeplitz_predict(ts[0], Zs[:, :c], Zs[:, :1], want_cov=True))[:4]
        return out

    before = earlier()
    clocks = h.times(), h.grad_times(), h.post_times()
    h.panel_times(reset=True)
    n = 2 * width() + 17
    rng = np.random.RandomState(5)
    t1 = tc.arfima_column(n, 0.4)
    gm.toeplitz_gram(t1, rng.randn(n, 33), 3, method="panel")
    gm.toeplitz_predict(t1, rng.randn(n, 33), rng.randn(n, 2), want_cov=True, method="panel")
    assert (h.times(), h.grad_times(), h.post_times()) == clocks
    ms = h.panel_times()
    assert tuple(ms) == _toep_lib.PANEL_PHASES and all(v > 0 for v in ms.values()), ms
    assert gc._same(earlier(), before)
    return ms


# ---- failures ---------------------------------------------------------------------------------------------------------------------------

def failure_positions(n):
    """toeplitz_cases.late_positions(n) and, with p the index of the edited entry (the recursion fails in step p - 1): the last step
    of a panel (p = j B), its first (j B + 1), the one after (j B + 2) and the one before the boundary (j B - 1), for the first
    boundary and one in the middle."""
    B = width()
    ps, p_nan = tc.late_positions(n)
    J = max(1, (n // B) // 2)
    ps = sorted(set(ps) | {j * B + o for j in {1, J} for o in (-1, 0, 1, 2) if 1 <= j * B + o <= n - 1})
    return ps, p_nan


def check_late_failures(backend, n, d=0.25):
    """toeplitz_cases.check_late_failures' construction at ``failure_positions(n)``: every failing column in one call around two
    healthy first columns; info == p + 1, NaN outputs, and the healthy ones bit-equal to a call of their own."""
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
    Z = tc.rhs_columns(n, 18)                                             # two 16-column tiles
    G0, s0, i0 = gm.toeplitz_gram(good, Z, 2, backend=backend, method="panel")
    G1, s1, i1 = gm.toeplitz_gram(other, Z, 2, backend=backend, method="panel")
    assert i0 == 0 and i1 == 0
    G, sld, info = gm.toeplitz_gram(np.stack([other] + bad[:half] + [good] + bad[half:] + [other]), Z, 2, backend=backend, method="panel")
    assert list(info) == [0] + want[:half] + [0] + want[half:] + [0], (n, list(info))
    healthy = [0, half + 1, len(info) - 1]
    rest = np.setdiff1d(np.arange(len(info)), healthy)
    assert np.isnan(sld[rest]).all() and np.isnan(G[rest]).all()
    assert np.array_equal(G[half + 1], G0) and sld[half + 1] == s0
    for i in (0, len(info) - 1):
        assert np.array_equal(G[i], G1) and sld[i] == s1
    # predict: info, NaN everywhere, no error
    K = tc.rhs_columns(n, 20, seed=2)
    for p in (ps[0], width(), width() + 1):
        r = gm.toeplitz_predict(bad[ps.index(p)], K, Z[:, :2], want_cov=True, backend=backend, method="panel")
        assert r.info == p + 1 and all(np.isnan(a).all() for a in (r.quad, r.cross, r.cov, r.G)) and np.isnan(r.sum_log_diag)
    return [int(x) for x in info]


# ---- the model layer --------------------------------------------------------------------------------------------------------------------

def surface_process(backend, n):
    """A truncation process on the grid 0.1 * arange(n) (the S2 / S3 inputs of test_gpu_toeplitz.py) and an 8 x 8 (length scale, ratio)
    surface's axes."""
    from sklearn.gaussian_process.kernels import RBF
    r = 4
    X = 0.1 * np.arange(n)[:, None]
    y = gm.partials(np.random.RandomState(0).randn(n, r), ratio=0.5, ref=1.0, orders=np.arange(r))
    gp = gm.TruncationGP(kernel=RBF(0.2), ratio=0.5, ref=1.0, center=0, disp=0, df=1, scale=1, optimizer=None, backend=backend)
    gp.X_train_, gp.y_train_, gp.orders_ = X, y, np.arange(r)
    return gp, [[v] for v in np.log(np.linspace(0.1, 0.3, 8))], list(np.linspace(0.3, 0.8, 8))


def check_surface(backend, n):
    """log_marginal_likelihood_grid(structure="toeplitz", toeplitz_method="panel") on an 8 x 8 surface: within rtol 1e-12 of the
    column route's surface (the rule that route's own surface is held to against its reference) with the same argmax."""
    gp, thetas, ratios = surface_process(backend, n)
    want = gp.log_marginal_likelihood_grid(thetas, ratios, structure="toeplitz")
    got = gp.log_marginal_likelihood_grid(thetas, ratios, structure="toeplitz", toeplitz_method="panel")
    assert got.shape == (8, 8) and np.isfinite(got).all()
    assert np.argmax(got) == np.argmax(want)
    np.testing.assert_allclose(got, want, rtol=1e-12)
    return float(np.max(np.abs(got - want) / np.abs(want)))


def check_model(backend, name, n):
    """The conjugate classes: log_marginal_likelihood and _batch without gradient take toeplitz_method; a fit with dense_factor=False
    remembers its toeplitz_method for predict and sample_y; every return form of predict within 1e-9 of the column route's and of the
    dense route's (the rule of toeplitz_post_cases.check_model between routes)."""
    import pytest
    cls, kw = gc.model_class(name), dict(gc.MODEL_CLASSES)[name]
    X, y = gc.model_xy(n)
    col = gc.model_process(cls, backend, optimizer=None, **kw).fit(X, y, structure="toeplitz", dense_factor=False)
    gp = gc.model_process(cls, backend, optimizer=None, **kw).fit(X, y, structure="toeplitz", dense_factor=False, toeplitz_method="panel")
    dense = gc.model_process(cls, backend, optimizer=None, **kw).fit(X, y)
    assert gp._toeplitz_method == "panel" and col._toeplitz_method == "columns" and gp.structure_ == "toeplitz"
    Xs = pc.new_points(X)
    calls = {"n": 0}
    from gsum_amd import toeplitz as tz
    real = tz.toeplitz_predict

    def spy(*a, **k):
        calls["n"] += 1
        calls["method"] = k.get("method")
        return real(*a, **k)

    worst = 0.0
    tz.toeplitz_predict = spy
    try:
        for call in pc.PREDICT_CALLS:
            out = pc._as_tuple(gp.predict(Xs, **call))
            assert calls["method"] == "panel", call
            for o, w, v in zip(out, pc._as_tuple(col.predict(Xs, **call)), pc._as_tuple(dense.predict(Xs, **call))):
                assert o.shape == w.shape and np.isfinite(o).all()
                worst = max(worst, float(np.max(np.abs(o - w)) / np.max(np.abs(w))))
                assert np.max(np.abs(o - w)) <= 1e-9 * np.max(np.abs(w)), call
                assert np.max(np.abs(o - v)) <= 1e-9 * np.max(np.abs(v)), call
            if call.get("return_cov"):
                assert np.array_equal(out[1], out[1].T)
        col.predict(Xs, return_std=True)
        assert calls["method"] == "columns"
        col.predict(Xs, return_std=True, toeplitz_method="panel")
        assert calls["method"] == "panel"
        draws = gp.sample_y(Xs, n_samples=2, random_state=4)
        assert calls["method"] == "panel" and np.isfinite(draws).all()
    finally:
        tz.toeplitz_predict = real
    with pytest.raises(ValueError, match="toeplitz_method"):
        gp.predict(Xs, toeplitz_method="bogus")
    with pytest.raises(ValueError, match="toeplitz_method"):
        gc.model_process(cls, backend, optimizer=None, **kw).fit(X, y, structure="toeplitz", toeplitz_method="bogus")
    thetas = list(gc.MODEL_THETAS)
    want = gp.log_marginal_likelihood_batch(thetas, structure="toeplitz")
    got = gp.log_marginal_likelihood_batch(thetas, structure="toeplitz", toeplitz_method="panel")
    np.testing.assert_allclose(got, want, rtol=1e-12)
    assert got[1] == gp.log_marginal_likelihood(thetas[1], structure="toeplitz", toeplitz_method="panel")
    with pytest.raises(ValueError, match="method"):
        gp.log_marginal_likelihood(thetas[1], structure="toeplitz", toeplitz_method="bogus")
    assert gp.fit(X, y)._toeplitz_method == "columns"                    # a later fit forgets it
    return worst
