"""Shared cases of the tiled Levinson replay of the Toeplitz path, ``method="blocked"`` on ``toeplitz_grad``, ``toeplitz_solve``,
``toeplitz_inverse_column``, ``toeplitz_inverse_diagonal`` and ``toeplitz_loo`` and ``toeplitz_grad_method="blocked"`` on the model
classes (test_toeplitz_levinson_cpu.py on backend='cpu', where the keyword selects nothing; test_gpu_toeplitz_levinson.py on 'hip'):
DESIGN.md section 24.

Up to n = 8192 the blocked method is held to the default one bit for bit: the coefficients come from the same pivot pairs through the
same step_coeffs, every element of A and B goes through the same rotate in the same order, and the kernels from x on are the same.
Beyond, the yardsticks are the exact identities of the pair dt = [t, e_0] and ARFIMA's closed-form inverse column
(toeplitz_grad_cases.identity_distances, here with the method as an argument) under toeplitz_cases._rule.  B (the panel width) and R
(the rows a tile owns) are asked of the library when a test runs.  Every check returns what it measured."""
import functools

import numpy as np

import gsum_amd as gm
import toeplitz_blocked_cases as bk
import toeplitz_cases as tc
import toeplitz_grad_cases as gc
from toeplitz_cases import EPS, FLOOR, LD, _rule

LIMIT = bk.LIMIT
PANEL_BUDGET = bk.PANEL_BUDGET
MODEL_SIZES = ("1", "2", "3", "B-1", "B", "B+1", "2B+1", "R-1", "R", "R+1", "R+B-1", "R+B", "R+B+1", "2R+17")
SMALL_GEOMETRIES = ((4, 12), (2, 3), (8, 8))         # (B, R) pairs at which the geometry, not the size, carries the model's test


def model_size(label, B, R):
    b, r, off = bk._EDGES[label]
    return b * B + r * R + off


# ---- the model of the tiled replay ------------------------------------------------------------------------------------------------------

def tiled_replay(rho, ic, B, R, halo=None, skip_top_tile=False):
    """A (n,) in long double after the n - 1 steps of Levinson's recursion from A = B = e_0, in k_levinson_tiles' geometry: panels of B
    steps; per panel the tiles 0 .. (its last step) // R of R own rows, each with ``halo`` rows loaded above them (B in the kernel;
    rows above row 0 are zeros, and the row a shift would bring into the halo's top is a zero: stale from then on); two state
    buffers, both zero-filled, read from one and written -- the own rows alone -- to the other.  The first panel always runs and takes
    A[0] = B[0] = 1.  ``skip_top_tile``: the variant whose panels leave out their top tile, where there is more than one."""
    n = len(rho) + 1
    halo = B if halo is None else halo
    cur, nxt = np.zeros((2, n), dtype=LD), np.zeros((2, n), dtype=LD)
    k0 = 0
    while True:
        k1 = min(k0 + B, n - 1)
        tiles = k1 // R + 1
        if skip_top_tile and tiles > 1:
            tiles -= 1
        for j in range(tiles):
            r0 = j * R
            rows = np.arange(r0 - halo, min(r0 + R, n))
            inside = rows >= 0
            a, b = np.zeros(len(rows), dtype=LD), np.zeros(len(rows), dtype=LD)
            a[inside], b[inside] = cur[0, rows[inside]], cur[1, rows[inside]]
            if k0 == 0:
                a[rows == 0] = b[rows == 0] = 1
            for k in range(k0 + 1, k1 + 1):                            # step k replays row k - 1
                bs = np.concatenate([np.zeros(1, dtype=LD), b[:-1]])
                a, b = (a - rho[k - 1] * bs) * ic[k - 1], (bs - rho[k - 1] * a) * ic[k - 1]
            nxt[0, rows[halo:]], nxt[1, rows[halo:]] = a[halo:], b[halo:]
        cur, nxt = nxt, cur
        k0 += B
        if not k0 < n - 1:
            return cur[0]


def replay_inputs(n, d=0.4):
    """(steps of ``_cpu_schur`` with the root, info, x of ``_cpu_inverse_column``) of the ARFIMA column."""
    from gsum_amd import toeplitz as tz
    t = tc.arfima_column(n, d)[None]
    steps = {}
    _, _, info = tz._cpu_schur(t, np.zeros((n, 1)), steps)
    steps["root"] = np.sqrt(t[:, 0].astype(LD))
    assert not info.any()
    return steps, info, tz._cpu_inverse_column(steps, info)[0]


def check_model(n, B, R):
    """The model on the coefficients of ``_cpu_schur`` equals the straight recursion of ``_cpu_inverse_column``, entry for entry."""
    steps, _, x = replay_inputs(n)
    scale = (steps["last"] * steps["root"])[0]
    got = tiled_replay(steps["rho"][0], steps["ic"][0], B, R) / scale
    assert got.dtype == LD and np.array_equal(got, x), (n, B, R, int(np.argmax(got != x)))
    return steps, scale, x


def check_model_variants_differ(n, B, R):
    """A halo one row short and a missing top tile both change the result: the model's test cannot pass on a wrong model."""
    steps, scale, x = check_model(n, B, R)
    short = tiled_replay(steps["rho"][0], steps["ic"][0], B, R, halo=B - 1) / scale
    topless = tiled_replay(steps["rho"][0], steps["ic"][0], B, R, skip_top_tile=True) / scale
    assert not np.array_equal(short, x), (n, B, R)
    assert not np.array_equal(topless, x), (n, B, R)


# ---- (1) bit for bit the one-workgroup route ----------------------------------------------------------------------------------------------

def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def all_pieces(t, dt, Z, backend, method, n_sets=1):
    """(G, sum_log_diag, info, trace, H, x, alpha, p) of one method, and the infos of the three other calls."""
    g = gm.toeplitz_grad(t, dt, Z, n_sets, backend=backend, method=method)
    x, ix = gm.toeplitz_inverse_column(t, backend=backend, method=method)
    al, ia = gm.toeplitz_solve(t, Z, backend=backend, method=method)
    p, ip = gm.toeplitz_inverse_diagonal(t, backend=backend, method=method)
    assert np.array_equal(ix, g[2]) and np.array_equal(ia, g[2]) and np.array_equal(ip, g[2])
    return tuple(g) + (x, al, p)


PIECES = ("G", "sum_log_diag", "info", "trace", "H", "x", "alpha", "p")


def check_equal_to_columns(backend, n):
    """(1): x, alpha, p, trace, H, sum_log_diag and info of ``method="blocked"`` are the default method's bit for bit on the two ARFIMA
    columns with dt = [t, e_0] and cols_at(n) right-hand sides, and G is ``toeplitz_gram(method="blocked")``'s."""
    t = bk.pn.arfima_columns(n)
    e0 = np.zeros(n)
    e0[0] = 1.0
    dt = np.stack([np.stack([ti, e0]) for ti in t])
    Z = tc.rhs_columns(n, gc.cols_at(n))
    blk, col = all_pieces(t, dt, Z, backend, "blocked"), all_pieces(t, dt, Z, backend, "columns")
    assert not blk[2].any() and np.isfinite(blk[5]).all()
    for k, name in enumerate(PIECES):
        if name != "G":
            assert np.array_equal(blk[k], col[k]), (n, name)
    Gv, sv, iv = gm.toeplitz_gram(t, Z, 1, backend=backend, method="blocked")
    assert np.array_equal(blk[0], Gv) and np.array_equal(blk[1], sv) and np.array_equal(blk[2], iv), n
    assert np.array_equal(blk[4], blk[4].transpose(0, 1, 2, 4, 3))
    return dict(sum_log_diag=[float(s) for s in blk[1]], x0=[float(v) for v in blk[5][:, 0]])


def golden_inputs(name):
    """(t, dt (1, n), Z) of an ill-conditioned golden with its length-scale derivative column (toeplitz_grad.npz)."""
    case = [c for c in gc.golden()["cases"] if c["name"] == name][0]
    t = tc.hex_column([c for c in tc.ill_cases() if c["name"] == name][0])
    return t, gc.golden_arrays()[name + "/dt"][None], tc.rhs_columns(case["n"], case["cols"])


def check_golden_equal_to_columns(backend, name):
    """(1): the same equalities on the ill-conditioned goldens, whose reflection coefficients come close to 1: the inputs that notice
    a lost low word (mutations)."""
    t, dt, Z = golden_inputs(name)
    blk, col = all_pieces(t, dt, Z, backend, "blocked"), all_pieces(t, dt, Z, backend, "columns")
    assert blk[2] == 0
    for k, what in enumerate(PIECES):
        if what != "G":
            assert np.array_equal(blk[k], col[k]), (name, what)
    Gv, sv, iv = gm.toeplitz_gram(t, Z, 1, backend=backend, method="blocked")
    assert np.array_equal(blk[0], Gv) and blk[1] == sv and blk[2] == iv, name
    return float(blk[3][0])


# ---- (2) beyond the limit ---------------------------------------------------------------------------------------------------------------

IDENTITY_D = tc.DS[0]
IDENTITY_KEYS = ("trace_t", "H_t", "trace_e0", "H_e0", "residual", "x", "p")
CPU_LIMIT = 8192 + 1024                              # the largest n at which the cpu backend sets the bound inside a test


@functools.lru_cache(maxsize=None)
def identity_distances(backend, n, method):
    """toeplitz_grad_cases.identity_distances with the method as an argument, one ARFIMA column (d = 0.4) and two right-hand sides,
    as that function arranges from n = 4095 on, and one piece more: diag(T^-1) against the closed-form x pushed through
    ``toeplitz_inverse_diagonal``'s formula in long double."""
    d = IDENTITY_D
    t = tc.arfima_column(n, d)
    e0 = np.zeros(n)
    e0[0] = 1.0
    dt = np.stack([t, e0])
    Z = tc.rhs_columns(n, 2)
    G, sld, info, trace, H, x, alpha, p = all_pieces(t, dt, Z, backend, method)
    assert info == 0 and G.shape == (1, 2, 2) and trace.shape == (2,) and H.shape == (1, 2, 2, 2) and x.shape == (n,) and alpha.shape == (n, 2)
    assert np.array_equal(H, H.transpose(0, 1, 3, 2))
    if backend != "cpu":                                                # on the cpu backend G is _cpu_gram's by construction
        Gv, sv, iv = gm.toeplitz_gram(t, Z, backend=backend, method=method)
        assert np.array_equal(G, Gv) and sld == sv and info == iv
    k = np.arange(n, dtype=LD)
    xt = gc.arfima_inverse_column(n, d)
    xn = np.concatenate([np.zeros(1, dtype=LD), xt[:0:-1]])
    pt = np.cumsum((xt - xn) * (xt + xn)) / xt[0]
    al = alpha.astype(LD)
    return dict(trace_t=float(abs(trace[0] - n) / n), H_t=gc.rel(H[0, 0], G[0]), trace_e0=gc.rel(trace[1], np.sum((n - 2 * k) * xt * xt) / xt[0]),
                H_e0=gc.rel(H[0, 1], al.T @ al), residual=gc.rel(gc.toeplitz_times_ld(t, al), Z, gc.toeplitz_times_ld(t, al, absolute=True)),
                x=gc.rel(x, xt), p=gc.rel(p, pt))


def check_identities_beyond(backend, n):
    """(2): every piece under the rule against the cpu backend's own distance (at most 4 x, floor 64 * 2^-53); from CPU_LIMIT on, where
    the cpu backend is too slow to run with every later change, under one floor: the least the rule can give."""
    got = identity_distances(backend, n, "blocked")
    cpu = identity_distances("cpu", n, "columns") if n <= CPU_LIMIT else None
    print(f"toeplitz levinson identities {backend} n={n}: " +
          ", ".join(f"{k} {got[k] / EPS:.2f}" + (f" (cpu {cpu[k] / EPS:.2f})" if cpu else "") for k in IDENTITY_KEYS) + ("" if cpu else " (cpu not run: one floor)"))
    for k in IDENTITY_KEYS:
        bound = _rule(cpu[k]) if cpu else FLOOR
        assert got[k] <= bound, (n, k, got[k] / EPS, bound / EPS)
    out = {k: got[k] / EPS for k in IDENTITY_KEYS}
    if cpu:
        out.update({"cpu_" + k: cpu[k] / EPS for k in IDENTITY_KEYS})
    return out


# ---- (3) independence and reproducibility -----------------------------------------------------------------------------------------------

def levinson_bytes(n, ncols, P):
    """The library's arithmetic (gsum_toep.hip: blocked_bytes + levinson_bytes) for ``toeplitz_grad(method="blocked")``: what the
    blocked route keeps per first column, then steps, the two states of A and B, xd, xf and the diagonal sums, and per entry of Z
    W, As and Q."""
    return bk.blocked_bytes(n, ncols) + (17 * n + n * ncols * (5 + 2 * P)) * 8


def first_columns_per_launch(n, ncols, P, m, budget=PANEL_BUDGET):
    return max(1, min(m, 65535, budget // levinson_bytes(n, ncols, P)))


def chunked_sets(n, c=16, P=1, m=3):
    """The least number of sets of c columns with which m = 3 first columns do not fit the budget together at order n."""
    n_sets = 1
    while first_columns_per_launch(n, n_sets * c, P, m) >= m:
        n_sets += 1
    return n_sets


def check_independence(backend, n):
    """(3): a (first column, set) result is bitwise unchanged under permuting the sets, halving them, padding with others, P = 1
    against 2 and a repeated call, and a column of alpha under the same of the columns; H is bitwise symmetric.  (Within a set H[a, b]
    is alpha_a^T (dT alpha_b) for a <= b, mirrored: the order of a set's own columns is part of its result, as on the default method.)"""
    rng = np.random.RandomState(7)
    t1 = tc.arfima_column(n, 0.4)
    e0 = np.zeros(n)
    e0[0] = 1.0
    dt2 = np.stack([np.cos(0.01 * np.arange(n)), e0])
    c, n_sets = 3, 4
    Zs = rng.randn(n_sets, n, c)

    def flat(sets):
        return sets.transpose(1, 0, 2).reshape(n, -1)

    def grad(sets, dt_=dt2):
        return gm.toeplitz_grad(t1, dt_, flat(sets), len(sets), backend=backend, method="blocked")

    def alpha(Z_):
        return gm.toeplitz_solve(t1, Z_, backend=backend, method="blocked")[0]

    full = grad(Zs)
    assert full[2] == 0 and np.array_equal(full[4], full[4].transpose(0, 1, 3, 2))
    assert _same(full, grad(Zs))                                                                             # the call repeated
    a_full = alpha(flat(Zs))
    for idx in (rng.permutation(n_sets), np.arange(0, n_sets, 2)):                                           # permuted, halved
        part = grad(Zs[idx])
        assert np.array_equal(part[0], full[0][idx]) and np.array_equal(part[4], full[4][idx]) and part[1] == full[1] and np.array_equal(part[3], full[3])
    cols = rng.permutation(n_sets * c)
    assert np.array_equal(alpha(flat(Zs)[:, cols]), a_full[:, cols]) and np.array_equal(alpha(flat(Zs)[:, ::2]), a_full[:, ::2])
    more = grad(np.concatenate([rng.randn(2, n, c), Zs, rng.randn(3, n, c)]))                                # padded with others
    sl = slice(2, 2 + n_sets)
    assert np.array_equal(more[0][sl], full[0]) and np.array_equal(more[4][sl], full[4]) and np.array_equal(more[3], full[3])
    assert np.array_equal(alpha(np.concatenate([rng.randn(n, 5), flat(Zs), rng.randn(n, 5)], axis=1))[:, 5:5 + n_sets * c], a_full)
    one = grad(Zs, dt2[:1])                                                                                  # P = 1 against 2
    assert _same(one[:3], full[:3]) and np.array_equal(one[3], full[3][:1]) and np.array_equal(one[4][:, :1], full[4][:, :1])
    x1, _ = gm.toeplitz_inverse_column(t1, backend=backend, method="blocked")
    xm, _ = gm.toeplitz_inverse_column(np.stack([tc.arfima_column(n, -0.3), t1]), backend=backend, method="blocked")
    assert np.array_equal(xm[1], x1)
    return float(full[1])


def check_chunk_loop(backend, n):
    """(3): three first columns that go through as two and one.  For each, G and H of the first, middle and last set, trace and
    sum_log_diag are bitwise those of a call with that first column and those three sets alone.  Device only."""
    c, P, m = 16, 1, 3
    n_sets = chunked_sets(n)
    assert first_columns_per_launch(n, n_sets * c, P, m) == 2 and first_columns_per_launch(n, (n_sets - 1) * c, P, m) == 3
    ts = np.stack([tc.arfima_column(n, d) for d in (0.4, -0.3, 0.25)])
    dts = np.stack([np.cos(0.01 * np.arange(n))[None]] * m)
    Z = np.asfortranarray(np.random.RandomState(11).standard_normal((n_sets * c, n)).T)
    got = gm.toeplitz_grad(ts, dts, Z, n_sets, backend=backend, method="blocked")
    assert not got[2].any()
    pick = [0, n_sets // 2, n_sets - 1]
    Z3 = np.concatenate([Z[:, s * c:(s + 1) * c] for s in pick], axis=1)
    for i in range(m):
        G1, s1, i1, tr1, H1 = gm.toeplitz_grad(ts[i], dts[i], Z3, 3, backend=backend, method="blocked")
        assert i1 == 0 and np.array_equal(got[0][i][pick], G1) and np.array_equal(got[4][i][pick], H1), i
        assert got[1][i] == s1 and np.array_equal(got[3][i], tr1), i
    return [int(v) for v in got[2]]


# ---- (4) failures -----------------------------------------------------------------------------------------------------------------------

def failure_positions(n):
    """The edited entries p (the recursion fails in step p - 1, info = p + 1): the first steps, around the first panel's end, around
    the first tile's end, around the limit of the default method, and the last two; and where the NaN goes."""
    B, R = bk.width(), bk.tile_rows()
    ps = [1, 2, B - 1, B, B + 1, R, R + 1, LIMIT, LIMIT + 1, n - 2, n - 1]
    return sorted({p for p in ps if 1 <= p <= n - 1}), min(n - 1, R + B + 3)


def check_failures(backend, n, d=0.25):
    """(4): t_p + 1.5 E_{p-1} of an ARFIMA column fails at step p + 1 exactly; a NaN in t at its step.  All failing first columns in one
    call between healthy ones: info is the value route's, the failed columns' x, alpha, p, trace and H are NaN, and the healthy ones
    come out bit for bit as they do in a call without the failed ones."""
    good, other = tc.arfima_column(n, d), tc.arfima_column(n, -0.3)
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
    ts = np.stack([other] + bad[:half] + [good] + bad[half:] + [other])
    healthy = [0, half + 1, len(ts) - 1]
    rest = np.setdiff1d(np.arange(len(ts)), healthy)
    Z = tc.rhs_columns(n, 2)
    dts = np.stack([np.cos(0.01 * np.arange(n))[None]] * len(ts))
    got = all_pieces(ts, dts, Z, backend, "blocked")
    assert list(got[2]) == [0] + want[:half] + [0] + want[half:] + [0], (n, list(got[2]))
    assert np.array_equal(got[2], gm.toeplitz_gram(ts, Z, 1, backend=backend, method="blocked")[2])          # as the value route gives it
    for k, name in enumerate(PIECES):
        if name != "info":
            assert np.isnan(got[k][rest]).all(), name
            assert np.isfinite(got[k][healthy]).all(), name
    alone = all_pieces(ts[healthy], dts[healthy], Z, backend, "blocked")
    assert _same([g[healthy] for g in got], alone)
    return [int(v) for v in got[2]]


# ---- (5) the other routes ---------------------------------------------------------------------------------------------------------------

def check_other_routes_undisturbed():
    """(5), device only: the value results of the three methods on toeplitz_cases.SHAPES and the default method's grad are bit-equal
    before and after blocked-gradient calls on the same handle, the five older clocks are not charged by them, and the new clock's
    eleven phases all are."""
    from gsum_amd import _toep_lib
    h = _toep_lib.default_handle(0)

    def earlier():
        out = []
        for ns, c, n_sets, m in tc.SHAPES:
            ts, Zs, _ = tc._kms_inputs(ns, c, n_sets, m)
            for method in ("columns", "panel", "blocked"):
                out += list(gm.toeplitz_gram(ts, Zs, n_sets, method=method))
            out += list(gm.toeplitz_grad(ts, np.stack([np.stack([np.arange(ns) * t]) for t in ts]), Zs, n_sets))
        return out

    before = earlier()
    clocks = h.times(), h.grad_times(), h.post_times(), h.panel_times(), h.blocked_times()
    h.levinson_times(reset=True)
    n = bk.tile_rows() + bk.width() + 17
    rng = np.random.RandomState(5)
    t1 = tc.arfima_column(n, 0.4)
    gm.toeplitz_grad(t1, np.cos(np.arange(n))[None], rng.randn(n, 33), 3, method="blocked")
    gm.toeplitz_loo(t1, rng.randn(n, 2), method="blocked")
    gm.toeplitz_inverse_column(t1, method="blocked")
    assert (h.times(), h.grad_times(), h.post_times(), h.panel_times(), h.blocked_times()) == clocks
    ms = h.levinson_times()
    assert tuple(ms) == _toep_lib.LEVINSON_PHASES and all(v > 0 for v in ms.values()), ms
    assert _same(earlier(), before)
    gm.toeplitz_grad(t1, np.cos(np.arange(n))[None], rng.randn(n, 3))                                          # nor the new clock by the old ones
    gm.toeplitz_gram(t1, rng.randn(n, 3), method="blocked")
    assert h.levinson_times() == ms
    return ms


# ---- (6) the model layer ------------------------------------------------------------------------------------------------------------------

def check_model_gradient_equal(backend, name, n):
    """(6): the [(lml, grad), ...] of log_marginal_likelihood_batch(eval_gradient=True, structure="toeplitz") with
    ``toeplitz_grad_method="columns"`` (which is the default's) and with ``"blocked"``, and the values of ``toeplitz_method="blocked"``."""
    gp = gc.model_process(gc.model_class(name), backend, optimizer=None, **dict(gc.MODEL_CLASSES)[name])
    X, y = gc.model_xy(n)
    thetas = list(gc.MODEL_THETAS)
    col = gp.log_marginal_likelihood_batch(thetas, X=X, y=y, structure="toeplitz", eval_gradient=True, toeplitz_grad_method="columns")
    blk = gp.log_marginal_likelihood_batch(thetas, X=X, y=y, structure="toeplitz", eval_gradient=True, toeplitz_grad_method="blocked")
    assert _grads_equal(col, gp.log_marginal_likelihood_batch(thetas, X=X, y=y, structure="toeplitz", eval_gradient=True))
    worst = max(max(abs(a[0] - b[0]) / abs(a[0]), float(np.max(np.abs(a[1] - b[1]) / np.abs(a[1])))) for a, b in zip(col, blk))
    print(f"toeplitz levinson model {backend} {name} n={n}: blocked against columns, worst relative difference of (lml, grad) {worst / EPS:.2f} * 2^-53")
    return col, blk, gp.log_marginal_likelihood_batch(thetas, X=X, y=y, structure="toeplitz", toeplitz_method="blocked")


def _grads_equal(a, b):
    return all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def beyond_process(backend, **kw):
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    return gm.ConjugateGaussianProcess(kernel=Matern(0.2, nu=0.5) + WhiteKernel(1e-6, noise_level_bounds="fixed"), backend=backend, center=0.1, disp=1.5,
                                       df=2, scale=0.7, **kw)


def ou_curves(n, length_scale=0.1, curves=2, seed=1):
    """Exact draws of the Matern-1/2 process with that length scale on n points of [0, 1] (an AR(1) chain), so that the calibration's
    optimum lies inside the kernel's bounds and the two fits of check_fit_beyond_the_limit are not both pinned to one."""
    e = np.random.RandomState(seed).randn(n, curves)
    phi = np.exp(-1.0 / ((n - 1) * length_scale))
    y = np.empty((n, curves))
    y[0] = e[0]
    for i in range(1, n):
        y[i] = phi * y[i - 1] + np.sqrt(1 - phi * phi) * e[i]
    return y


def check_fit_beyond_the_limit(backend, n=LIMIT + 1, q=5):
    """(6): a default-optimiser fit with both keywords ``"blocked"`` and no dense factor at n = 8193, then predict(return_std=True) and
    loo(): finite and of the right shapes; the optimum's objective value within 100 factr eps (toeplitz_grad_cases.check_fit's bound)
    of the optimum of the same fit on the first 8192 points with the default gradient method, re-evaluated at n = 8193 on the value
    route; loo bit for bit ``toeplitz_loo(method="blocked")`` called directly."""
    X = np.linspace(0, 1, n)[:, None]
    y = ou_curves(n)
    gp = beyond_process(backend).fit(X, y, structure="toeplitz", dense_factor=False, toeplitz_method="blocked", toeplitz_grad_method="blocked")
    assert gp.structure_ == "toeplitz" and gp._toeplitz_method == "blocked" and gp.corr_L_ is None and gp._fit_grad_method == "columns"
    v = gp.log_marginal_likelihood_value_
    assert np.isfinite(v) and np.isfinite(gp.kernel_.theta).all()
    Xs = np.linspace(0.05, 0.95, q)[:, None] + 0.37 / n
    mean, std = gp.predict(Xs, return_std=True)
    assert mean.shape == (q, 2) and std.shape == (q,) and np.isfinite(mean).all() and np.isfinite(std).all() and (std > 0).all()
    loo = gp.loo()
    for a, shape in ((loo.mean, (n, 2)), (loo.var, (n,)), (loo.error, (n, 2)), (loo.logpdf, (n, 2)), (loo.precision_diag, (n,))):
        assert a.shape == shape and np.isfinite(a).all()
    t = gm.toeplitz_column(gp.kernel_, X, gp.nugget, backend=backend)
    direct = gm.toeplitz_loo(float(np.squeeze(gp.cov_factor_)) * t, y, gp.mean(X), backend=backend, method="blocked")
    assert _same(loo, direct)
    ref = beyond_process(backend).fit(X[:LIMIT], y[:LIMIT], structure="toeplitz", dense_factor=False, toeplitz_method="blocked")
    v_ref = float(gp.log_marginal_likelihood_batch([ref.kernel_.theta], X=X, y=y, structure="toeplitz", toeplitz_method="blocked")[0])
    diff = abs(v - v_ref) / abs(v_ref)
    print(f"toeplitz levinson fit {backend} n={n}: length scale {np.exp(gp.kernel_.theta)[0]:.6g} (n={LIMIT}: {np.exp(ref.kernel_.theta)[0]:.6g}), value {v!r}, "
          f"the n={LIMIT} optimum at n={n} {v_ref!r}, relative difference {diff:.3g}")
    lo, hi = np.exp(gp.kernel_.bounds[0])
    assert lo * 10 < np.exp(gp.kernel_.theta)[0] < hi / 10                                                   # an optimum inside the bounds
    assert diff <= 100 * gc.FACTR_EPS, (v, v_ref)
    return diff
