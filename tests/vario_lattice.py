"""Lattice designs for the variogram and a truth for its cov sums that is independent of both backends (no GPU, no device library).

The lattice: X = arange(N)[:, None], bounds = arange(0.5, N - 1), optionally padded with repeats of 1e6 (non-decreasing; the extra
bins stay empty).  Every distance is an exact integer, bin k (k = 1 .. N - 1) holds exactly the N - k pairs (i, i - k) in tril order
(i ascending), bin 0 is empty, and the bin of points a, b is |a - b|.  So
    counts == [0, N - 1, .., 1],  h_sum[k] == k (N - k) exactly in any summation order,
    dij_sum[k, a] == [a >= k] + [a + k < N] exactly for the indicator curve of point a (sqrt|1 - 0| = 1, sqrt|0 - 0| = 0).

gamma~ for the cov stage is an input: the rational model gt[k, c] = nugget_c + sill_c k / (k + ell_c) uses only + * /, so every
machine reproduces its bits (exp would not).  It is > 0 everywhere, bin 0 included.

The truth.  For pair p = (i, i - k1) of bin k1 against q = (k, k - k2) of bin k2, rho depends only on the offset s = i - k:
    rho(s) = (((g[|s - k1|] + g[|s + k2|]) - g[|s|]) - g[|s - k1 + k2|]) / (2 sqrt(g[k1] g[k2]))
in float64 in exactly this order: the device's num / dn (k_cov).  Swapping the two bins maps s to -s and exchanges only the two
operands of the first addition, so the bits do not depend on which bin the device puts on its lanes.  The sum over a bin pair is
sum_s mult(s) corr(rho(s)) sq with mult(s) = #{i : k1 <= i < N, k2 <= i - s < N} from integer counting; for k1 == k2 the s == 0
terms (p == q) are 1 sq.  corr is mpmath's corr_factor (2F1(-1/4, -1/4; 1/2; rho^2) - 1) at 30 digits with the +-1 clamps.
"""
import base64
import hashlib
from collections import namedtuple
from math import gamma

import numpy as np

VAR_FACTOR = 2. / np.pi * (np.sqrt(np.pi) - gamma(0.75)**2)          # VariogramFourthRoot.var_factor, corr_factor
CORR_FACTOR = gamma(0.75)**2 / (np.sqrt(np.pi) - gamma(0.75)**2)

# curve c of variant 0; variant 1 (the request-list cache's second gamma~) has other ell_c and sill_c
ELL = [3., 17., 60., 250., 900., 7., 33., 120., 480.]
SILL = [1., 0.5, 2., 0.75, 1.5, 1.25, 0.25, 3., 0.625]
NUGGET = [0.01, 0.02, 0.005, 0.03, 0.015, 0.025, 0.002, 0.04, 0.0125]

EDGE_BINS = [87, 88, 89, 343, 344, 345, 598, 599]                    # N = 600: 513, 512, 511, 257, 256, 255, 2, 1 pairs


def lattice(N, n_bounds=None):
    """X and bounds; n_bounds > N - 1 pads with repeats of 1e6."""
    X = np.arange(N, dtype=float)[:, None]
    bounds = np.arange(0.5, N - 1)
    if n_bounds is not None:
        assert n_bounds >= len(bounds)
        bounds = np.concatenate([bounds, np.full(n_bounds - len(bounds), 1e6)])
    return X, bounds


def counts_exact(N, nbin=None):
    c = np.zeros(nbin or N, dtype=np.int64)
    c[1:N] = N - np.arange(1, N)
    return c


def h_sum_exact(N, nbin=None):
    h = np.zeros(nbin or N)
    k = np.arange(1, N)
    h[1:N] = k * (N - k)
    return h


def indicator_dij_exact(N, points, nbin=None):
    """dij_sum[k, a] of the indicator curves of ``points``: [a >= k] + [a + k < N] for 1 <= k < N, 0 in the empty bins"""
    a = np.asarray(points)[None, :]
    k = np.arange(nbin or N)[:, None]
    return np.where((k >= 1) & (k < N), (a >= k).astype(float) + (a + k < N), 0.)


def model_gt(nbin, nc, variant=0):
    """gt[k, c] = nugget_c + sill_c k / (k + ell_c), float64, one operation at a time"""
    k = np.arange(nbin, dtype=float)[:, None]
    ell, sill, nug = (np.array(v[:nc])[None, :] for v in (ELL, SILL, NUGGET))
    if variant == 1:
        ell, sill = 2. * ell + 1., 0.5 * sill + 0.25
    return nug + (sill * k) / (k + ell)


def n_tiles(m1, m2, same, tile=256):
    """tiles k_cov evaluates for one request of bins with m1, m2 pairs"""
    t1, t2 = -(-m1 // tile), -(-m2 // tile)
    if not (m1 and m2):
        return 0
    return t1 * (t1 + 1) // 2 if same else t1 * t2


def rho_offsets(g, k1, k2, N):
    """(rho(s), mult(s), s) of one gamma~ column g for the bins k1, k2 >= 1 of the lattice, every offset with mult > 0"""
    s = np.arange(k1 - (N - 1), (N - 1) - k2 + 1)
    mult = np.minimum(N - 1, N - 1 + s) - np.maximum(k1, k2 + s) + 1
    assert mult.min() >= 1 and mult.sum() == (N - k1) * (N - k2)
    num = ((g[np.abs(s - k1)] + g[np.abs(s + k2)]) - g[np.abs(s)]) - g[np.abs(s - k1 + k2)]
    return num / (2 * np.sqrt(g[k1] * g[k2])), mult, s


def sq_of(g, k1, k2):
    """sqrt(var1 var2), var = var_factor sqrt(gamma~), in the order of gsum_vario_cov and _cpu_cov_sum"""
    return np.sqrt((VAR_FACTOR * np.sqrt(g[k1])) * (VAR_FACTOR * np.sqrt(g[k2])))


def _mp_corr():
    import mpmath as mp
    mp.mp.dps = 30
    g2 = mp.gamma(mp.mpf(3) / 4) ** 2
    cf = g2 / (mp.sqrt(mp.pi) - g2)
    cache = {}

    def corr(r):
        r = float(r)
        if r >= 1:
            return mp.mpf(1)
        if r <= -1:
            return mp.mpf(-1)
        r = abs(r)                                                   # even in rho inside (-1, 1)
        if r not in cache:
            cache[r] = cf * (mp.hyp2f1(-0.25, -0.25, 0.5, mp.mpf(r) ** 2) - 1)
        return cache[r]
    return mp, corr


def truth(gt, N, requests):
    """Per request (k1, k2) and curve: dict of arrays (n_requests, nc): ``sum`` (the truth, rounded once to double), ``E`` =
    sum mult |term|, ``sq``, ``sens`` = the change of the sum when every rho moves one ulp up, or one ulp down, whichever is larger,
    and ``M`` (n_requests,) = the number of (p, q) terms.  A request with bin 0 (empty) is all zeros.  Needs mpmath."""
    mp, corr = _mp_corr()
    nc = gt.shape[1]
    out = {k: np.zeros((len(requests), nc)) for k in ("sum", "E", "sq", "sens")}
    out["M"] = np.zeros(len(requests), dtype=np.int64)
    for r, (k1, k2) in enumerate(requests):
        if k1 == 0 or k2 == 0:
            continue
        out["M"][r] = (N - k1) * (N - k2)
        for c in range(nc):
            g = np.ascontiguousarray(gt[:, c])
            rho, mult, s = rho_offsets(g, k1, k2, N)
            sq = sq_of(g, k1, k2)
            tot = E = up = dn = mp.mpf(0)
            for rh, m, ss in zip(rho, mult, s):
                m = int(m)
                if k1 == k2 and ss == 0:
                    t = mp.mpf(1)
                else:
                    t = corr(rh)
                    up += m * (corr(np.nextafter(rh, np.inf)) - t)
                    dn += m * (corr(np.nextafter(rh, -np.inf)) - t)
                tot += m * t
                E += m * abs(t)
            sqm = mp.mpf(float(sq))
            out["sum"][r, c] = float(tot * sqm)
            out["E"][r, c] = float(E * sqm)
            out["sens"][r, c] = float(max(abs(up), abs(dn)) * sqm)
            out["sq"][r, c] = sq
    return out


# ---- the cases of tests/golden/vario_lattice_truth.json ---------------------------------------------------------------------------
DIAG = [(k, k) for k in EDGE_BINS]
OFF = [(343, 344), (88, 345), (87, 599), (344, 599)]
GROUP_REQUESTS = [(343, 343), (344, 345), (87, 599)]
CACHE_A = [(343, 344), (88, 88), (599, 87)]
CACHE_B = [(88, 345), (599, 599), (344, 599)]
LDS_REQUESTS = [(119, 119), (60, 60), (1, 1), (1, 60)]               # bins of 1, 60 and 119 pairs
CAP_REQUESTS = [(2098, 2098), (2098, 1844)]                          # 2 pairs; 2 x 256 pairs

# name -> (N, curves, gamma~ variant, requests with k1 <= k2; the other order has the same truth)
CASES = {
    "tiles": (600, 5, 0, DIAG + OFF),
    "groups": (600, 9, 0, GROUP_REQUESTS),
    "cache_second_gamma": (600, 2, 1, [tuple(sorted(r)) for r in CACHE_A]),
    "lds": (120, 4, 0, LDS_REQUESTS),
    "cap": (2100, 3, 0, [tuple(sorted(r)) for r in CAP_REQUESTS]),
}
GT_STORED_UP_TO = 600 * 9              # gt itself is stored up to this many entries (the file's size limit); its SHA-256 always


def L(a):
    a = np.array(a, dtype="<f8", order="C")
    return {"f64": base64.b64encode(a.tobytes()).decode(), "shape": list(a.shape)}


def A(v):
    return np.frombuffer(base64.b64decode(v["f64"]), "<f8").reshape(v["shape"])


def gt_digest(gt):
    return hashlib.sha256(np.ascontiguousarray(gt, dtype="<f8").tobytes()).hexdigest()


def make_fixture():
    """The whole fixture as a dict (needs mpmath).  gt is the model on the lattice's own bins 0 .. N - 1: no request reads another."""
    cases = {}
    for name, (N, nc, variant, requests) in CASES.items():
        gt = model_gt(N, nc, variant)
        t = truth(gt, N, requests)
        rec = dict(N=N, nc=nc, variant=variant, requests=[list(r) for r in requests], gt_sha256=gt_digest(gt),
                   M=[int(m) for m in t["M"]], **{k: L(t[k]) for k in ("sum", "E", "sq", "sens")})
        if gt.size <= GT_STORED_UP_TO and name != "tiles":           # tiles: the first five columns of the groups case's gt
            rec["gt"] = L(gt)
        cases[name] = rec
    return dict(cases=cases)


Row = namedtuple("Row", "sum E sq sens M")          # one request: arrays over the curves, M the number of (p, q) terms


class Truth:
    """One fixture case: ``row(k1, k2)`` is the request's Row, either order of the bins, zeros (M = 0) for an empty bin."""

    def __init__(self, rec):
        self.rec = rec
        self.N, self.nc = rec["N"], rec["nc"]
        self.idx = {tuple(r): n for n, r in enumerate(rec["requests"])}
        self.arr = {k: A(rec[k]) for k in ("sum", "E", "sq", "sens")}
        self.M = rec["M"]

    def row(self, k1, k2):
        if k1 == 0 or k2 == 0:
            z = np.zeros(self.nc)
            return Row(z, z, z, z, 0)
        n = self.idx[(min(k1, k2), max(k1, k2))]
        return Row(*(self.arr[k][n] for k in ("sum", "E", "sq", "sens")), self.M[n])

    def atol(self, k1, k2):
        """4e-15 sq M (the device correlation map's asserted distance from mpmath, every term) + sens + (264 + tiles) 2^-53 E: any
        summation order of at most 256 loop steps per lane, the 8 levels of the 256-wide tree and the chain of tile partials in
        k_cov_reduce.  sens is the change of the whole sum when every rho moves one ulp the same way (the larger of up and down):
        a division biased by an ulp.  corr is even in rho, so the per-term changes partly cancel in it; it does not bound a
        division that errs either way term by term (that is sum mult |change|, larger).  The device's division is correctly
        rounded, and the term is below a twentieth of the first."""
        t = self.row(k1, k2)
        if not t.M:
            return np.zeros(self.nc)
        m1, m2 = self.N - k1, self.N - k2
        return 4e-15 * t.sq * t.M + t.sens + (264 + n_tiles(m1, m2, k1 == k2)) * 2.0 ** -53 * t.E
