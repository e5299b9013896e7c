"""Cases, long-double truth and error measures for libgsum_pointwise.so at its launch edges (no tests here): what
tests/test_pointwise_edges_cpu.py and tests/test_gpu_pointwise_edges.py share.

Three families, each aimed at an index or a partition of kernels/pointwise.hip.h that a benign input cannot pin:

* coverage (``k_coverage``): intervals across the blocks of kCovD = 128 (blockIdx.y), 1 / 63 / 64 kept orders in the LDS table, one
  tile / many tiles / a second strided trip of a workgroup.  Exact int64 counts of numpy's own expression; the inputs make every
  counter differ from its neighbours and plant the points a compare can get wrong (on a bound, NaN, +-inf, scale 0 / < 0 / inf).
* one-hot rows (``k_differences``, ``k_loglike``, ``k_loglike_rows``): a background of points whose addend is exactly +0.0 and one or
  two planted points, so the row's output is the planted point's own output bit for bit, whatever the order of the sum.
* the grid likelihood against a long-double truth in five order regimes (benign, one order, 64 orders, negative orders, sparse
  orders with a middle one excluded), at n on both sides of the 1024-point segment and of the 64th partial.

Everything is seeded and built in memory; nothing is read from a file.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

import gsum_amd as gm
from grad_truth import EPS, LD, _require_extended  # noqa: F401  (re-exported: the test files take them from here)
from pointwise_common import LOGLIKE_RTOL

REF_CAP = LOGLIKE_RTOL / 16          # every likelihood case: float64 itself sits this far inside the bound (asserted on the cpu)
REF_SCALAR, REF_POINTS, REF_ROW_SCALAR, REF_ROW_POINTS = range(4)      # gsum_pointwise.h: GSUM_POINTWISE_REF_*


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


# ---- 1. coverage ------------------------------------------------------------------------------------------------------------------

# (n, kp, D): D across kCovD at kp = 5; kp = 1, 63, 64 (64 x 128 fills the LDS table, 64 x 129 runs a second block with nd = 1);
# n across the wave, the tile and, with 524289 = 256 * 2048 + 1, the second strided trip of one workgroup with one live lane
COVERAGE_SHAPES = ([(257, 5, D) for D in (1, 127, 128, 129, 256, 257)] + [(257, 1, 129), (257, 63, 129), (257, 64, 128), (257, 64, 129)]
                   + [(n, 5, 129) for n in (1, 63, 64, 65, 255, 256, 524289)])
COVERAGE_CASES = [(n, kp, D, dc) for n, kp, D in COVERAGE_SHAPES for dc in sorted({1, kp})]
PLANT_MIN_N = 64                     # the special points are planted from this n on
DISTINCT_MIN_N = 255                 # from this n on no two rows and no two columns of the expected table are equal
PLANTS = ("data_nan", "loc_nan", "scale_nan", "data_pinf", "data_ninf", "scale_zero", "scale_negative", "scale_inf",
          "on_lower", "on_lower", "on_lower", "on_lower", "on_upper", "on_upper", "on_upper", "on_upper")


def coverage_expected(loc, scale, data, t_lo, t_hi):
    """The cpu expression of TruncationPointwise._coverage_counts: (D, kp) int64."""
    with np.errstate(invalid="ignore"):              # 0 * inf: NaN, which compares false, is the point
        return np.stack([np.sum((lo * scale + loc < data) & (data < hi * scale + loc), axis=0) for lo, hi in zip(t_lo, t_hi)]).astype(np.int64)


def fused_bound(t, s, l):
    """t * s + l rounded once (what a contracted multiply-add would give), by exact rational arithmetic."""
    return float(Fraction(float(t)) * Fraction(float(s)) + Fraction(float(l)))


@dataclass
class CoverageCase:
    n: int
    kp: int
    D: int
    loc: np.ndarray                   # (n, kp)
    scale: np.ndarray                 # (n, kp)
    t_lo: np.ndarray                  # (D,)
    t_hi: np.ndarray
    data: dict                        # data_cols -> (n, data_cols)
    expected: dict = field(default_factory=dict)      # data_cols -> (D, kp) int64
    plants: list = field(default_factory=list)        # (kind, point, column, interval or None)

    def counts(self, data_cols):
        """the expected (D, kp) table of a data layout, computed once (at n = 524289 a table costs seconds)"""
        if data_cols not in self.expected:
            self.expected[data_cols] = coverage_expected(self.loc, self.scale, self.data[data_cols], self.t_lo, self.t_hi)
        return self.expected[data_cols]

    def distinct(self, data_cols):
        """no two rows and no two columns of the expected table are equal"""
        table = self.counts(data_cols)
        return len({r.tobytes() for r in table}) == table.shape[0] and len({c.tobytes() for c in table.T}) == table.shape[1]


def _duplicate_rows(tables):
    """the rows that repeat an earlier row in any of the tables"""
    out = set()
    for table in tables:
        seen = set()
        for d, row in enumerate(table):
            key = row.tobytes()
            if key in seen:
                out.add(d)
            seen.add(key)
    return sorted(out)


def _draw_coverage(n, kp, D, attempt):
    rng = np.random.RandomState(_seed("coverage", n, kp, D, attempt))
    col = np.geomspace(0.3, 3.0, kp) if kp > 1 else np.ones(1)                       # every column its own scale
    loc0 = rng.standard_normal((n, kp)) + np.linspace(-0.5, 0.5, kp)
    scale0 = col * rng.uniform(0.5, 1.5, (n, kp))
    data0 = {1: 1.5 * rng.standard_normal((n, 1))}
    data0[kp] = data0[1] if kp == 1 else loc0 + scale0 * 1.2 * rng.standard_normal((n, kp))
    # the intervals: drawn one by one, neither nested nor sorted; one lower and one upper quantile are exactly 0 (0 * inf = NaN)
    zero_lo, zero_hi = D // 2, (D // 3 if D >= 3 else None)

    def draw(d):
        if d == zero_lo:
            return 0.0, rng.uniform(0.05, 4.0)
        if d == zero_hi:
            return -rng.uniform(0.05, 3.0), 0.0
        lo = rng.uniform(-3.0, 1.5)
        return lo, lo + rng.uniform(0.05, 4.0)

    t = np.array([draw(d) for d in range(D)])
    spots = [(n * (2 * q + 1)) // (2 * len(PLANTS)) for q in range(len(PLANTS))] if n >= PLANT_MIN_N else []
    assert len(set(spots)) == len(spots)
    for _ in range(400):
        loc, scale, data = loc0.copy(), scale0.copy(), {dc: a.copy() for dc, a in data0.items()}
        plants = []
        for kind, i in zip(PLANTS, spots):
            j = i % kp
            d = None
            if kind == "data_nan":
                data[1][i, 0] = data[kp][i, j] = np.nan
            elif kind == "loc_nan":
                loc[i, j] = np.nan
            elif kind == "scale_nan":
                scale[i, j] = np.nan
            elif kind in ("data_pinf", "data_ninf"):
                data[1][i, 0] = data[kp][i, j] = np.inf if kind == "data_pinf" else -np.inf
            elif kind == "scale_zero":
                scale[i, :] = 0.0
            elif kind == "scale_negative":
                scale[i, :] = -scale[i, :]
            elif kind == "scale_inf":
                scale[i, :] = np.inf
            else:
                # data exactly on the twice-rounded bound of interval d, column j; the point's scale is nudged until a bound rounded
                # once would lie on the other side of it, so that a contracted multiply-add counts the point and this table does not
                d = (7 * i + 3) % D
                tq = t[d, 0] if kind == "on_lower" else t[d, 1]
                for step in range(256):
                    s = scale0[i, j] * (1.0 + step / 4096.0)
                    bound = tq * s + loc[i, j]
                    fused = fused_bound(tq, s, loc[i, j])
                    if tq == 0.0 or (fused < bound if kind == "on_lower" else fused > bound):
                        break
                scale[i, j] = s
                data[1][i, 0] = data[kp][i, j] = bound
            plants.append((kind, i, j, d))
        if not DISTINCT_MIN_N <= n <= 4096:                         # larger: 5-vectors of counts up to n do not collide; the cpu test asserts it
            expected = {}
            break
        expected = {dc: coverage_expected(loc, scale, a, t[:, 0], t[:, 1]) for dc, a in data.items()}
        dups = _duplicate_rows(expected.values())
        if not dups:
            break
        for d in dups:
            t[d] = draw(d)
    return CoverageCase(n, kp, D, loc, scale, t[:, 0].copy(), t[:, 1].copy(), data, expected, plants)


@functools.lru_cache(maxsize=None)
def coverage_case(n, kp, D):
    """The case of a shape, both data layouts ((n, 1) and (n, kp)) on the same loc, scale and intervals, with its expected counts."""
    for attempt in range(32):
        case = _draw_coverage(n, kp, D, attempt)
        if not DISTINCT_MIN_N <= n <= 4096 or all(case.distinct(dc) for dc in case.data):
            return case
    raise AssertionError(f"no coverage case with distinct counters at n={n} kp={kp} D={D}")


def coverage_handle_inputs(kp):
    """(orders, mask) of a handle that keeps kp orders (the coverage does not read the orders themselves)"""
    return np.arange(kp, dtype=np.int32), np.ones(kp, dtype=np.int32)


def credible_inputs(backend):
    """(model, data, dobs): credible_diagnostic at n = 1025 with 257 degrees of belief, three interval blocks through the public call"""
    p = problem("benign", 1025)
    m = p.model(backend)
    data = p.y[:, -1] + 3 * np.median(m.dist_.kwds["scale"]) * np.random.RandomState(1025).standard_normal(1025)
    return m, data, np.linspace(0, 1, 257)


# ---- the truth of one row ------------------------------------------------------------------------------------------------------------

def differences(y):
    """y_j - y_{j-1} (y_0 itself for column 0) with one float64 rounding: numpy.diff, as series.coefficients and k_differences take it"""
    y = np.asarray(y, dtype=np.float64)
    c = np.empty(y.shape)
    c[:, 0] = y[:, 0]
    c[:, 1:] = np.diff(y, axis=-1)
    return c


def jac_per_point(ratio, ref):
    """the change-of-variables term is summed over what ratio and ref broadcast to: once for two scalars, else per point"""
    return np.ndim(ratio) > 0 or np.ndim(ref) > 0


def truth_row(dy, orders, ratio, ref, df0, scale0):
    """(T, M) of one row in long double.  dy: (n, kp) float64 differences of the kept columns (exact inputs); orders: the kp kept
    orders; ratio, ref: a scalar or (n,).  T = sum_i 0.5 df log((df0 scale0^2 + sum_j c_ij^2) / 2) + the change of variables
    log|ref| + S log ratio, counted once for scalar ratio and ref and per point otherwise; M is the same sum over absolute values
    (loglike_magnitude without the constants, which the library's raw output does not carry)."""
    _require_extended()
    dy = np.asarray(dy, dtype=np.float64)
    n, kp = dy.shape
    o = np.asarray(orders, dtype=np.int64).astype(LD)
    r = np.asarray(ratio, dtype=np.float64).astype(LD)
    f = np.asarray(ref, dtype=np.float64).astype(LD)
    with np.errstate(all="ignore"):
        c = dy.astype(LD) / (np.reshape(f, (-1, 1)) * np.reshape(r, (-1, 1)) ** o)
        df = LD(df0) + LD(kp)
        s = LD(df0) * (LD(scale0) * LD(scale0)) + np.sum(c * c, axis=1)
        points = LD(0.5) * df * np.log(s / LD(2))
        jac = np.log(np.abs(f)) + np.sum(o) * np.log(r)
        if jac_per_point(ratio, ref):               # a point's two terms are one addend, as on the device
            T = np.sum(points + jac)
            M = np.sum(np.abs(points)) + np.sum(np.abs(np.broadcast_to(jac, (n,))))
        else:
            T = np.sum(points) + jac
            M = np.sum(np.abs(points)) + np.abs(jac)
    return T, float(M)


def f64_row(y, orders, mask, ratio, ref, df0, scale0):
    """The reference's numpy expression of the same quantity in float64 (TruncationPointwise._log_likelihood_host without its constants,
    sign flipped): coefficients with ``**``, scale through its square root, df log(df scale^2 / 2)."""
    orders, mask = np.asarray(orders), np.asarray(mask, dtype=bool)
    with np.errstate(all="ignore"):
        c = gm.coefficients(y=y, ratio=ratio, ref=ref, orders=orders)[:, mask]
        df = df0 + c.shape[-1]
        scale = np.sqrt((df0 * scale0 ** 2 + (c ** 2).sum(-1)) / df)
        return 0.5 * np.sum(df * np.log(df * scale ** 2 / 2.)) + np.sum(np.log(np.abs(ref)) + np.sum(orders[mask]) * np.log(ratio))


def rel_error(value, T, M):
    """|value - T| / M, the subtraction in long double"""
    return float(abs(LD(value) - T) / LD(M))


# ---- 2. one-hot rows -----------------------------------------------------------------------------------------------------------------

ONEHOT_SIZES = (1025, 2049, 65537)
ONEHOT_ORDERS = np.array([0, 1])
ONEHOT_DF0, ONEHOT_SCALE0 = 0.0, 1.0
PLANT_DIFF, PLANT_RATIO, PLANT_REF = (1.5, -0.75), 0.7, -1.3
RATIO_KINDS = ("G", "Gn")
REF_KINDS = ("scalar", "n", "G", "Gn")
ONEHOT_G = 3


def onehot_positions(n):
    """lane 0, the last lane of a wave, the first of the next, the last and first of a thread's stride, the last and first of a
    segment, and the last point (at 65537: the one live lane of the 65th partial)"""
    return [0, 63, 64, 255, 256, 1023, 1024, n - 1]


def onehot_calls(n):
    """(p, qs): the point whose differences are planted and the point of each of the three rows that carries the per-point ratio /
    ref plant.  One of the rows has q = p (one-hot), the others two planted points; which row it is rotates.  The two planted points
    of a row never belong to one thread of k_loglike (the cpu test asserts it), so each reaches the sum as a rounded addend of its own."""
    P = onehot_positions(n)
    calls = []
    for k in range(len(P)):
        qs = [P[k], P[(k + 3) % 8], P[(k + 5) % 8]]
        calls.append((P[k], tuple(qs[-(k % 3):] + qs[:-(k % 3)]) if k % 3 else tuple(qs)))
    return calls


def onehot_signs(n):
    """the background's first differences (+-1, +-1), a fixed pattern"""
    i = np.arange(n)
    return np.where(i % 3 == 0, -1.0, 1.0), np.where((i // 2) % 2 == 0, 1.0, -1.0)


def onehot_y(n, p):
    """(n, 2) partial sums whose first differences are the background's everywhere and PLANT_DIFF at p; every difference is exact"""
    d0, d1 = onehot_signs(n)
    d0[p], d1[p] = PLANT_DIFF
    y = np.stack([d0, d0 + d1], axis=1)
    assert np.array_equal(differences(y), np.stack([d0, d1], axis=1))
    return y


def onehot_operands(n, p, qs, ratio_kind, ref_kind):
    """(ratios, refs, ref_mode, points): the operands of a call and, per row, the planted points as (d0, d1, ratio, ref) tuples.
    A per-row operand is planted at the row's q, a shared (n,) ref at p; a (G,) or scalar operand cannot carry a plant and is 1."""
    G = len(qs)
    d0, d1 = onehot_signs(n)
    ratios = np.ones(G) if ratio_kind == "G" else np.ones((G, n))
    if ratio_kind == "Gn":
        for g, q in enumerate(qs):
            ratios[g, q] = PLANT_RATIO
    if ref_kind == "scalar":
        refs, mode = np.ones(1), REF_SCALAR
    elif ref_kind == "G":
        refs, mode = np.ones(G), REF_ROW_SCALAR
    elif ref_kind == "n":
        refs, mode = np.ones(n), REF_POINTS
        refs[p] = PLANT_REF
    else:
        refs, mode = np.ones((G, n)), REF_ROW_POINTS
        for g, q in enumerate(qs):
            refs[g, q] = PLANT_REF
    points = []
    for g, q in enumerate(qs):
        row = []
        for i in sorted({p, q}):
            ratio = ratios[g, i] if ratio_kind == "Gn" else 1.0
            ref = refs[i] if ref_kind == "n" else refs[g, i] if ref_kind == "Gn" else 1.0
            d = PLANT_DIFF if i == p else (d0[i], d1[i])
            if i == p or ratio != 1.0 or ref != 1.0:
                row.append((float(d[0]), float(d[1]), float(ratio), float(ref)))
        points.append(row)
    return ratios, refs, mode, points


def single_operands(point, ratio_kind, ref_kind):
    """(y, ratios, refs, ref_mode) of the n = 1, G = 1 call of the same mode that holds ``point`` alone"""
    d0, d1, ratio, ref = point
    y = np.array([[d0, d0 + d1]])
    ratios = np.array([ratio]) if ratio_kind == "G" else np.array([[ratio]])
    refs = np.array([[ref]]) if ref_kind == "Gn" else np.array([ref])
    mode = {"scalar": REF_SCALAR, "n": REF_POINTS, "G": REF_ROW_SCALAR, "Gn": REF_ROW_POINTS}[ref_kind]
    return y, ratios, refs, mode


def row_operands(ratios, refs, ref_kind, g):
    """(ratio, ref) of row g as log_likelihood and truth_row take them: a scalar or (n,)"""
    ratio = ratios[g]
    ref = refs[0] if ref_kind == "scalar" else refs if ref_kind == "n" else refs[g]
    return (float(ratio) if np.ndim(ratio) == 0 else ratio), (float(ref) if np.ndim(ref) == 0 else ref)


# ---- 3. the grid likelihood in five order regimes -------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Regime:
    orders: tuple
    excluded: tuple
    df0: float
    scale0: float
    fit_ratio: tuple                  # (a, b): a + b x over x in [0, 1]
    grid_ratios: tuple                # three (a, b), one per row
    sizes: tuple


SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2049)
LONG_SIZES = SIZES + (65536, 65537)
REGIMES = {
    "benign": Regime(tuple(range(6)), (0,), 0.6, 0.8, (0.25, 0.2), ((0.2, 0.3), (0.35, 0.1), (0.5, -0.25)), LONG_SIZES),
    "one": Regime((0, 3), (0,), 0.6, 0.8, (0.25, 0.2), ((0.2, 0.3), (0.35, 0.1), (0.5, -0.25)), SIZES),
    "sixty-four": Regime(tuple(range(65)), (0,), 1.0, 1.0, (0.8, 0.3), ((0.7, 0.6), (0.75, 0.5), (1.2, -0.4)), SIZES),
    # c reaches 1e40 and beyond, c^2 and their sum stay finite
    "sixty-four/small": Regime(tuple(range(65)), (0,), 1.0, 1.0, (0.3, 0.0), ((0.05, 0.05), (0.06, 0.04), (0.1, -0.03)), SIZES),
    "negative": Regime(tuple(range(-3, 4)), (), 0.6, 0.8, (1.2, 0.5), ((1.1, 0.6), (1.5, 0.25), (2.0, -0.8)), SIZES),
    "sparse": Regime((0, 2, 3, 7, 40), (2,), 0.0, 1.0, (0.6, 0.3), ((0.5, 0.4), (0.7, 0.2), (0.95, -0.3)), LONG_SIZES),
}
LIKELIHOOD_CASES = [(name, n) for name, reg in REGIMES.items() for n in reg.sizes]
MODE_SIZES = (1025, 65537)            # all eight ratio x ref modes, benign
MODE_CASES = [(n, rk, fk) for n in MODE_SIZES for rk in RATIO_KINDS for fk in REF_KINDS]


@dataclass
class Problem:
    name: str
    n: int
    y: np.ndarray                     # (n, k)
    orders: np.ndarray
    mask: np.ndarray                  # bool (k,)
    excluded: list
    df0: float
    scale0: float
    fit_ratio: np.ndarray             # (n,)
    fit_ref: np.ndarray               # (n,)
    ratios: np.ndarray                # (3, n)
    x: np.ndarray

    @property
    def dy(self):
        return differences(self.y)[:, self.mask]

    @property
    def kept(self):
        return self.orders[self.mask]

    def model(self, backend):
        m = gm.TruncationPointwise(df=self.df0, scale=self.scale0, excluded=self.excluded or None, backend=backend)
        with np.errstate(invalid="ignore"):          # a fitted ratio of exactly 1 has no geometric tail (dist_ only; the likelihood is unaffected)
            return m.fit(self.y, ratio=self.fit_ratio, ref=self.fit_ref, orders=self.orders)


@functools.lru_cache(maxsize=None)
def problem(name, n):
    reg = REGIMES[name]
    rng = np.random.RandomState(_seed("likelihood", name, n))
    x = np.linspace(0, 1, n) if n > 1 else np.array([0.5])
    orders = np.array(reg.orders)
    fit_ratio = reg.fit_ratio[0] + reg.fit_ratio[1] * x
    fit_ref = 1.5 + np.cos(3 * x)
    coeffs = rng.standard_normal((n, len(orders)))
    if name == "sixty-four/small":
        # every fourth point starts at order 40: its partial sums stay small enough for the late differences (0.3^64 = 3e-34) not to
        # be rounded away, and against a grid ratio of 0.05 their c reaches 1e49
        coeffs[::4, :40] = 0.0
    y = gm.partials(coeffs, ratio=fit_ratio, ref=fit_ref, orders=orders)
    ratios = np.stack([a + b * x for a, b in reg.grid_ratios])
    return Problem(name, n, y, orders, ~np.isin(orders, reg.excluded), list(reg.excluded), reg.df0, reg.scale0, fit_ratio, fit_ref, ratios, x)


@functools.lru_cache(maxsize=None)
def likelihood_truth(name, n):
    """[(T, M, out_f64)] of the three rows of a case with the fitted (n,) ref: the truth, its magnitude, the float64 expression"""
    p = problem(name, n)
    return [truth_row(p.dy, p.kept, p.ratios[g], p.fit_ref, p.df0, p.scale0)
            + (float(f64_row(p.y, p.orders, p.mask, p.ratios[g], p.fit_ref, p.df0, p.scale0)),) for g in range(len(p.ratios))]


def mode_operands(n, ratio_kind, ref_kind):
    """(problem, ratios, refs, ref_mode) of a benign case in one of the eight modes, three rows that all differ"""
    p = problem("benign", n)
    rng = np.random.RandomState(_seed("modes", n, ratio_kind, ref_kind))
    G = 3
    ratios = np.array([0.27, 0.41, 0.58]) if ratio_kind == "G" else p.ratios
    if ref_kind == "scalar":
        refs, mode = np.array([1.7]), REF_SCALAR
    elif ref_kind == "n":
        refs, mode = p.fit_ref, REF_POINTS
    elif ref_kind == "G":
        refs, mode = np.array([1.7, -2.3, 0.6]), REF_ROW_SCALAR
    else:
        refs, mode = rng.uniform(1, 3, (G, n)) * np.where(rng.uniform(size=(G, n)) < 0.25, -1.0, 1.0), REF_ROW_POINTS
    return p, ratios, refs, mode


@functools.lru_cache(maxsize=None)
def mode_truth(n, ratio_kind, ref_kind):
    p, ratios, refs, _ = mode_operands(n, ratio_kind, ref_kind)
    out = []
    for g in range(3):
        ratio, ref = row_operands(ratios, refs, ref_kind, g)
        out.append(truth_row(p.dy, p.kept, ratio, ref, p.df0, p.scale0) + (float(f64_row(p.y, p.orders, p.mask, ratio, ref, p.df0, p.scale0)),))
    return out


# ---- classes, not values -------------------------------------------------------------------------------------------------------------

CLASS_N = 1025


def value_class(v):
    v = float(v)
    return "nan" if np.isnan(v) else "+inf" if v == np.inf else "-inf" if v == -np.inf else "finite"


def class_cases():
    """name -> (df0, y, orders, excluded, fit ratio, fit ref, ratios (G,) or (G, n), refs None or (G,) or (G, n), expected classes):
    the inputs on which the result leaves the finite numbers.  Expected classes are the reference's own, worked out by hand here and
    compared with backend='cpu' in the cpu test."""
    n = CLASS_N
    p = problem("benign", n)
    base = (p.y, p.orders, p.excluded, p.fit_ratio, p.fit_ref)
    rows = p.ratios
    cases = {}
    y0 = p.y.copy()
    y0[700, :] = y0[700, 0]                                          # kept differences all exactly zero at one point, df0 = 0: log 0
    cases["log_zero"] = (0.0, y0) + base[1:] + (rows, None, ["+inf"] * 3)
    neg = rows.copy()
    neg[1, 1024] = -0.3                                              # log of a negative ratio: NaN in that row only
    cases["negative_ratio"] = (0.6,) + base + (neg, None, ["finite", "nan", "finite"])
    cases["negative_ratio_scalar"] = (0.6,) + base + (np.array([0.3, -0.3, 0.4]), np.array([1.0, 2.0, 3.0]), ["finite", "nan", "finite"])
    zero = rows.copy()
    zero[2, 0] = 0.0                                                 # c = inf, log inf = inf; S log 0 = -inf: inf - inf
    cases["zero_ratio"] = (0.6,) + base + (zero, None, ["finite", "finite", "nan"])
    cases["zero_ratio_scalar"] = (0.6,) + base + (np.array([0.0, 0.3, 0.4]), np.array([1.0, 2.0, 3.0]), ["nan", "finite", "finite"])
    tiny = rows.copy()
    tiny[0, :] = 1e-50                                               # ratio^5 = 1e-250 is a normal number; c ~ 1e247, c * c overflows
    cases["overflow"] = (0.6,) + base + (tiny, None, ["-inf", "finite", "finite"])
    refs = np.broadcast_to(p.fit_ref, (3, n)).copy()
    refs[1, 1023] = np.nan
    cases["nan_ref"] = (0.6,) + base + (rows, refs, ["finite", "nan", "finite"])
    return cases


def class_model(case, backend):
    df0, y, orders, excluded, fit_ratio, fit_ref = case[:6]
    return gm.TruncationPointwise(df=df0, scale=0.8, excluded=excluded, backend=backend).fit(y, ratio=fit_ratio, ref=fit_ref, orders=orders)
