"""Cholesky factors that every arithmetic order reproduces bit for bit, their closed-form consumers, and the checks built on them
(designs, expectations and helper functions; no tests here).

A design is (n, partition, seed).  {0 .. n-1} is split into "source" indices S1 and "sink" indices S2:
  alt       even indices are S1: every 16 x 16 diagonal micro-block has sub-diagonal content
  blocks16  (i // 16) % 2 == 0 is S1: diagonal micro-blocks are diagonal, off-diagonal ones dense (the complement of alt)
  rand      Bernoulli 1/2, seeded, index 0 in S1
N is strictly lower triangular with N[i, j] in {-2, -1, 1, 2} with probability 0.3 where i in S2, j in S1, j < i, and 0 elsewhere; every
S2 row with an S1 column to its left has at least one nonzero.  N maps S1 into S2 only, so N^2 = 0, and so is the square of every
principal sub-block of N.  With e_i in {-2 .. 5}, D = diag(2^e_i):

    L = (I + N) D,   A = L L^T,   L^-1 = D^-1 (I - N)

and the inverse of every diagonal sub-block of L is the same expression on that sub-block (the 16 x 16 micro-block inverses of the
substitution tables, the 128 x 128 blocks of Linv).  Every pivot is 4^e_i, every Schur complement an integer multiple of 2^-4, and for
integer Z, Y, mean in [-3, 3] every entry of L, L^-1, W = L^-1 Z, G = W^T W, X = L^-T W, L Z, E = L^-1 (Y - mean) and md2 = sum E^2 is a
dyadic rational of few bits.  The expectations are the closed forms in float64:

    W = D^-1 (I - N) Z,   X = (I - N)^T D^-1 W,   sld = ln 2 * sum e_i

EXACTNESS IS A CONDITION OF A DESIGN, checked here on the CPU (``Design.check``): for every product the device (or LAPACK) forms --
|L| |L|^T, |L^-1| |Z|, |W| |L|^T, |W|^T |W|, |L^-T| |W|, |L|^T |X|, |L| |Z|, |E|^T |E| -- the sum of the absolute values of the terms of
every entry is formed, with the number of fractional bits of the terms; integer bits of the largest such sum plus fractional bits must
stay <= 53.  Then every partial sum of every entry, in any order of summation, fused or not, is a multiple of the common unit below
2^53 units: representable, so no operation rounds.  A design that does not meet this raises.  A itself is also recomputed in int64.

WHY THE DEVICE IS EXPECTED TO BE EXACT AS WELL.  The only operations of the factorisation that are not sums of products are the
reciprocal square root of a pivot and what gs_potf2_16 derives from it.  gs_rsqrt_nr(p) for p = 4^k: h = p / 2 is a power of two, so
h r is exact for every r; a Newton step computes e = 0.5 - h r^2 with one rounding (one fma of the exact h r with r) and then r (1 + e)
(another fma).  From any hardware estimate with relative error below about 2^-14 the first step lands on 2^-k or on the number one
ulp below it (the error after the step is 1.5 d^2 < 2^-27 relative, far inside one ulp, and the result of the fma is the rounding of a
number that close to 2^-k); the second step maps both to exactly 2^-k (from 2^-k: e = 0, r unchanged; from 2^-k (1 - 2^-53): e = 2^-53
up to a term of 2^-106 that the fma sees and the rounding of r (1 + e) drops).  So d0 = p0 r0 = 2^k exactly, its correction term
p0 - d0^2 is zero, and l10 = a10 r0, r1, d1, m0, m1 are products with powers of two: exact.  q = p0 p1r - a10^2 and its kin are single
fmas whose exact result is representable.  Everything else -- the trailing updates, the substitutions against the micro-block
inverses, the Gram corner, L Z, the row sums of squares -- is MFMA or FMA accumulation of dyadic values within 53 bits (above).

sld IS THE ONLY INEXACT OUTPUT: each log(2^e) is within one ulp (2 eps |e| ln 2, eps = 2^-53), and the order of the n - 1 additions is
not fixed ((n - 1) eps sum |e_i| ln 2 to first order, for every order): |sld - ln 2 sum e_i| <= eps (n + 1) ln 2 sum |e_i|.  Derived,
not measured (the second-order terms are below 1e-12 of it at n <= 2100).  Any structural mistake -- a block's partial sum dropped or
taken twice, a pad row counted -- moves sld by at least ln 2.
"""
from __future__ import annotations

import math
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

PARTITIONS = ("alt", "blocks16", "rand")
EXPONENTS = (-2, 5)                     # e_i in -2 .. 5 inclusive
GSUM_MAX_RHS = 16
EPS = 2.0 ** -53
# ln 2 to 60 digits (public constant), as an exact rational: the truth sld is compared with
LN2 = Fraction(int("693147180559945309417232121458176568075500134360255254120680"), 10 ** 60)

# the orders of section 1 (640 / 641: the padding goes from 128 to 256 and the persistent chain begins) and their rotating partitions
ORDERS = (1, 2, 15, 16, 17, 127, 128, 129, 255, 256, 257, 383, 384, 385, 640, 641, 767, 768, 769, 1023, 1024, 1025, 1537, 2100)
OPERATOR_CASES = tuple((n, PARTITIONS[i % 3]) for i, n in enumerate(ORDERS))
SCHEDULE_ORDERS = (385, 640, 641, 1025, 1537, 2100)
SWEEP_ORDERS, SWEEP_COLUMNS = (897, 1025, 2100), (1023, 1024, 1100)
SWEEP_CASES = tuple((n, k) for n in SWEEP_ORDERS for k in SWEEP_COLUMNS)      # section 3: n = 897 pads to 1024, T = 8: the sweeps' own thresholds
INFO_ORDERS = (641, 1025, 1537)
INFO_COLUMNS = (0, 15, 16, 127, 128, 255, 256, 511, 512, 767, 768, -1)       # -1: n - 1
SEQUENCE_ORDERS = (385, 1025)


def _bits(x):
    """integer bits of max |x| (0 for zero)"""
    m = float(np.max(np.abs(x))) if np.size(x) else 0.0
    return 0 if m < 1.0 else int(math.floor(math.log2(m))) + 1


def _frac_bits(x):
    """the smallest f with x * 2^f integer in every entry"""
    x = np.asarray(x, dtype=float)
    for f in range(0, 64):
        y = x * 2.0 ** f
        if np.array_equal(y, np.rint(y)):
            return f
    raise AssertionError("not dyadic within 63 fractional bits")


def product_bits(X, Y):
    """Bits any summation order of X @ Y needs: integer bits of max (|X| |Y|) plus the fractional bits of a term."""
    S = np.abs(X) @ np.abs(Y)
    return _bits(S) + _frac_bits(X) + _frac_bits(Y)


class Design:
    """One exact factor with its closed forms.  ``e`` (n,) exponents, ``N`` (n, n), ``L``, ``A`` float64; ``bits``: what ``check`` found."""

    def __init__(self, n, partition, seed, N, e):
        self.n, self.partition, self.seed = int(n), partition, int(seed)
        self.N, self.e = N, e
        self.d = np.ldexp(1.0, e)                              # diag(D)
        self.L = (np.eye(n) + N) * self.d[None, :]
        self.A = self.L @ self.L.T
        self.bits = {}
        self._check_factor()

    # ---- closed forms ------------------------------------------------------------------------------------------------------------
    def linv(self):
        return (np.eye(self.n) - self.N) / self.d[:, None]

    def W(self, Z):
        Z = np.asarray(Z, dtype=float)
        return (Z - self.N @ Z) / self.d[:, None]

    def G(self, Z):
        W = self.W(Z)
        return W.T @ W

    def X(self, B):
        V = self.W(B) / self.d[:, None]
        return V - self.N.T @ V

    def LZ(self, Z):
        return self.L @ np.asarray(Z, dtype=float)

    def sld_exact(self):
        return LN2 * int(self.e.sum())

    def sld_bound(self):
        return EPS * (self.n + 1) * math.log(2.0) * float(np.abs(self.e).sum())

    def check_sld(self, sld):
        """|sld - ln 2 sum e| in exact arithmetic against the derived bound; returns the error as a float."""
        err = abs(Fraction(float(sld)) - self.sld_exact())
        assert err <= Fraction(self.sld_bound()), (float(err), self.sld_bound(), self.n)
        return float(err)

    # ---- exactness conditions ----------------------------------------------------------------------------------------------------
    def _need(self, name, bits):
        self.bits[name] = max(bits, self.bits.get(name, 0))
        assert bits <= 53, f"design (n={self.n}, {self.partition}, seed={self.seed}): {name} needs {bits} bits"

    def _check_factor(self):
        from scipy.sparse import csr_matrix
        n = self.n
        assert np.array_equal(self.N, np.tril(self.N, -1))
        assert not (self.N @ self.N).any()                      # N^2 = 0
        self._need("|L||L|^T", product_bits(self.L, self.L.T))
        # A with all scalings applied, in int64: L 2^s is an integer matrix for s = -min(e, 0) + fractional bits of N
        s = _frac_bits(self.L)
        Li = csr_matrix(np.rint(self.L * 2.0 ** s).astype(np.int64))
        Ai = (Li @ Li.T).toarray()
        assert np.abs(Ai).max() < 2 ** 53
        assert np.array_equal(self.A * 4.0 ** s, Ai.astype(float)), "A = L L^T is not exact in float64"
        assert np.array_equal(self.A, self.A.T)
        assert np.array_equal(self.linv() @ self.L, np.eye(n))

    def check(self, Z=None, B=None, Y=None, mean=None):
        """The exactness conditions of the consumers for these operands (each integer valued); raises where one is not met."""
        Li = self.linv()
        if Z is not None:
            Z = np.asarray(Z, dtype=float)
            assert np.array_equal(Z, np.rint(Z))
            W = self.W(Z)
            self._need("|L^-1||Z|", product_bits(Li, Z))
            self._need("|W||L|^T", product_bits(W.T, self.L.T))
            self._need("|W|^T|W|", product_bits(W.T, W))
            self._need("|L||Z|", product_bits(self.L, Z))
        if B is not None:
            B = np.asarray(B, dtype=float)
            W, X = self.W(B), self.X(B)
            self._need("|L^-1||Z|", product_bits(Li, B))
            self._need("|W||L|^T", product_bits(W.T, self.L.T))
            self._need("|L^-T||W|", product_bits(Li.T, W))
            self._need("|L|^T|X|", product_bits(self.L.T, X))
        if Y is not None:
            R = np.asarray(Y, dtype=float) - (0.0 if mean is None else np.asarray(mean, dtype=float)[:, None])
            assert np.array_equal(R, np.rint(R))
            E = self.W(R)
            self._need("|L^-1||Z|", product_bits(Li, R))
            self._need("|W||L|^T", product_bits(E.T, self.L.T))
            self._need("|E|^T|E|", _bits((E * E).sum(0)) + 2 * _frac_bits(E))
        return self


def _sources(n, partition, rng):
    i = np.arange(n)
    if partition == "alt":
        return i % 2 == 0
    if partition == "blocks16":
        return (i // 16) % 2 == 0
    if partition == "rand":
        s = rng.random(n) < 0.5
        s[0] = True
        return s
    raise ValueError(partition)


@lru_cache(maxsize=6)
def design(n, partition, seed=0, emin=EXPONENTS[0]):
    rng = np.random.default_rng([int(n), PARTITIONS.index(partition), int(seed)])
    s1 = _sources(n, partition, rng)
    allowed = np.tril(~s1[:, None] & s1[None, :], -1)
    vals = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=(n, n))
    N = np.where(allowed & (rng.random((n, n)) < 0.3), vals, 0.0)
    for i in np.nonzero(allowed.any(1) & ~N.any(1))[0]:         # every sink row with a source to its left has at least one nonzero
        j = np.nonzero(allowed[i])[0][-1]
        N[i, j] = vals[i, j]
    e = rng.integers(emin, EXPONENTS[1] + 1, size=n)
    d = Design(n, partition, seed, N, e)
    d.s1 = s1
    return d


def operands(n, k, seed):
    """integer right-hand sides in [-3, 3]"""
    return np.random.default_rng([int(n), int(k), int(seed)]).integers(-3, 4, size=(n, k)).astype(float)


def operator_inputs(d):
    """The operands of section 1 for a design, their exactness checked: Z (n x 16: k = 1, 5, 16 are its leading columns), B (n x 20), Y (n x 3), mean."""
    n = d.n
    Z, B, Y = operands(n, 16, 1), operands(n, 20, 2), operands(n, 3, 3)
    mean = operands(n, 1, 4)[:, 0]
    d.check(Z=Z, B=B, Y=Y, mean=mean)
    return Z, B, Y, mean


def failing(d, cols, twice=False):
    """A with A_jj lowered by 4^e_j (pivot j exactly 0) -- ``twice``: by 2 * 4^e_j (pivot -4^e_j) -- for every j of cols: potrf reports
    min(cols) + 1.  The Schur complements left of column j are the design's own, so everything up to the failing pivot is exact."""
    A = d.A.copy()
    for j in cols:
        A[j, j] -= (2.0 if twice else 1.0) * d.d[j] ** 2
    return A


@lru_cache(maxsize=4)
def guard_design(n, refused):
    """Row j (a sink) with pivot exactly 1 under A_jj = 2^51 + 1 (two entries 2^25 in its row of L: p <= gs_pivot_guard A_jj = 1 + 2^-51
    with the default guard of 2 ulps: refused, info j + 1) or under A_jj = 2^50 + 1 (one entry 2^25: the threshold is 1/2 + 2^-51:
    accepted).  Exponents >= 0 so that A is integer; the factor's exactness conditions hold for it like for every design."""
    base = design(n, "rand", 11, emin=0)
    N, e = base.N.copy(), base.e.copy()
    s2 = np.nonzero(~(np.abs(N).sum(0) > 0) & (np.abs(N).sum(1) > 0))[0]            # sinks: rows with content, empty columns
    j = int(s2[s2 < n - 3][-1])
    src = np.nonzero(np.abs(N).sum(0) > 0)[0]
    c = src[src < j][-2:]
    assert len(c) == 2
    N[j, :] = 0.0
    e[j] = 0
    for col in (c if refused else c[:1]):
        N[j, col] = 2.0 ** 25 / 2.0 ** e[col]
    g = Design(n, "rand", 11, N, e)
    assert g.L[j, j] == 1.0 and g.A[j, j] == (2.0 ** 51 if refused else 2.0 ** 50) + 1.0
    return g, j


# ---- Fraction arithmetic (small orders) -----------------------------------------------------------------------------------------------
def _fsqrt(q):
    a, b = math.isqrt(q.numerator), math.isqrt(q.denominator)
    assert a * a == q.numerator and b * b == q.denominator, q
    return Fraction(a, b)


def fraction_reference(A, Z):
    """(L, W, X, G) of A = L L^T, W = L^-1 Z, X = L^-T W, G = W^T W in exact rational arithmetic (right-looking Cholesky, zeros skipped)."""
    n, k = Z.shape
    a = [[Fraction(float(A[i, j])) for j in range(i + 1)] for i in range(n)]
    Lf = [[Fraction(0)] * n for _ in range(n)]
    for j in range(n):
        dj = _fsqrt(a[j][j])
        Lf[j][j] = dj
        col = [(i, a[i][j] / dj) for i in range(j + 1, n) if a[i][j] != 0]
        for i, li in col:
            Lf[i][j] = li
        for p, (i, li) in enumerate(col):
            for (q, lq) in col[:p + 1]:
                a[i][q] -= li * lq
    W = [[Fraction(int(Z[i, c])) for c in range(k)] for i in range(n)]
    for i in range(n):
        for c in range(k):
            s = W[i][c]
            for j in range(i):
                if Lf[i][j] != 0:
                    s -= Lf[i][j] * W[j][c]
            W[i][c] = s / Lf[i][i]
    X = [row[:] for row in W]
    for i in range(n - 1, -1, -1):
        for c in range(k):
            s = X[i][c]
            for j in range(i + 1, n):
                if Lf[j][i] != 0:
                    s -= Lf[j][i] * X[j][c]
            X[i][c] = s / Lf[i][i]
    G = [[sum(W[i][a_] * W[i][b_] for i in range(n)) for b_ in range(k)] for a_ in range(k)]
    f = lambda M: np.array([[float(x) for x in row] for row in M], dtype=float).reshape(len(M), -1)      # noqa: E731
    for M in (Lf, W, X, G):
        for row in M:
            for x in row:
                assert Fraction(float(x)) == x                 # representable: float() above did not round
    return f(Lf), f(W), f(X), f(G)


# ---- the checks, shared by the cpu backend (tests/test_exact_factors_cpu.py) and the device (tests/test_gpu_exact_factors.py) ----------
def eq(got, want):
    np.testing.assert_array_equal(np.asarray(got), np.asarray(want))


def check_factor(ctx, d, A=None):
    """upload, potrf, to_host against the design; returns the resident factor (the caller frees it)."""
    A = d.A if A is None else A
    M = ctx.upload(A)
    try:
        eq(M.to_host(), A)
        assert ctx.potrf(M) == 0
        Lg = M.to_host()
        eq(np.triu(Lg, 1), 0.0)
        eq(Lg, d.L)
    except BaseException:
        M.free()
        raise
    return M


def check_gram(ctx, M, d, Z):
    G, sld = ctx.forward_gram(M, Z)
    eq(G, d.G(Z))
    return d.check_sld(sld)


def check_operators(ctx, d, record=None):
    """Section 1: every operator on one design, every output against its closed form."""
    Z, B, Y, mean = operator_inputs(d)
    M = check_factor(ctx, d)
    try:
        errs = [check_gram(ctx, M, d, Z[:, :k]) for k in (1, 5, 16)]
        eq(ctx.forward_solve(M, Z), d.W(Z))
        eq(ctx.forward_solve(M, Z[:, 0]), d.W(Z[:, :1])[:, 0])
        eq(ctx.cho_solve(M, B), d.X(B))                         # 20 columns: two device passes
        eq(ctx.tri_multiply(M, B), d.LZ(B))
        E, m2 = ctx.sqrt_errors(M, Y, mean, pivot=False, md2=True)
        Ew = d.W(Y - mean[:, None])
        eq(E, Ew)
        eq(m2, (Ew * Ew).sum(0))
        E0, m0 = ctx.sqrt_errors(M, Y[:, :0], mean, pivot=False, md2=True)
        assert np.shape(E0) == (d.n, 0) and np.shape(m0) == (0,)
        eq(M.to_host(), d.L)                                    # and nothing of it moved the factor
    finally:
        M.free()
    if record is not None:
        record(f"exact_sld_n{d.n}_{d.partition}", sld_abs_err=max(errs), bound=d.sld_bound(), bits=max(d.bits.values()))


def info_cases(n):
    """(columns lowered, twice) of section 4 at order n: every column of INFO_COLUMNS alone with a zero AND with a negative pivot (the
    diagonal kernel eliminates columns in pairs and refuses even and odd columns by different expressions), and two pairs (the smaller
    index is reported)."""
    cols = sorted({(n - 1 if j < 0 else j) for j in INFO_COLUMNS if j < n})
    out = [((j,), twice) for j in cols for twice in (False, True)]
    out.append(((cols[len(cols) // 2], cols[2]), False))
    out.append(((cols[-1], cols[3]), True))
    return out


def check_info(ctx, d, cols, twice):
    M = ctx.upload(failing(d, cols, twice))
    try:
        info = ctx.potrf(M)
        assert info == min(cols) + 1, (info, cols, twice, d.n)
        assert not M.factored
    finally:
        M.free()


def check_sequences(ctx, n):
    """Section 5: call sequences on one factor; after every step the result is that of the call on a fresh factor (the closed form)."""
    d1, d2 = design(n, "rand", 5), design(n, "rand", 6)
    Z = operands(n, 5, 21)
    Zp = Z.copy()
    Zp[n // 2, 3] += 1.0                                        # the same k, one entry changed
    B = operands(n, 16, 22)
    Y = operands(n, 3, 23)
    for dd in (d1, d2):
        dd.check(Z=Z, B=B, Y=Y)
        dd.check(Z=Zp, B=Z)
    M1, M2 = check_factor(ctx, d1), check_factor(ctx, d2)

    def gram(M, dd, z):
        check_gram(ctx, M, dd, z)

    def solve(M, dd, z):
        eq(ctx.forward_solve(M, z), dd.W(z))

    def cho(M, dd, b):
        eq(ctx.cho_solve(M, b), dd.X(b))

    try:
        gram(M1, d1, Z); gram(M1, d1, Z)                                            # noqa: E702  (a remembered solve: the same answer)
        gram(M1, d1, Z); gram(M1, d1, Zp); gram(M1, d1, Z)                          # noqa: E702  (one entry changed: no stale hit)
        gram(M1, d1, Z); solve(M1, d1, Z[:, :4])                                    # noqa: E702  (k = 5, then k = 4 of the same columns)
        solve(M1, d1, Z); cho(M1, d1, Z); solve(M1, d1, Z); gram(M1, d1, Z)         # noqa: E702  (cho_solve overwrites the held solve)
        gram(M1, d1, Z)
        E, m2 = ctx.sqrt_errors(M1, Y, None, pivot=False, md2=True)
        eq(E, d1.W(Y)); eq(m2, (d1.W(Y) ** 2).sum(0))                               # noqa: E702
        gram(M1, d1, Z)
        gram(M1, d1, Z); eq(ctx.tri_multiply(M1, B), d1.LZ(B)); eq(M1.to_host(), d1.L); gram(M1, d1, Z)      # noqa: E702
        # two factors on one context: the shared upload buffer remembers the last right-hand sides of EITHER
        gram(M1, d1, Z); gram(M2, d2, Zp); gram(M1, d1, Z); cho(M2, d2, Z); gram(M2, d2, Zp)      # noqa: E702
        gram(M2, d2, Z); gram(M1, d1, Z); solve(M2, d2, Z); solve(M1, d1, Zp)       # noqa: E702
        # the same host array object, modified in place between two calls
        buf = Z.copy()
        gram(M1, d1, buf)
        buf[:] = Zp
        gram(M1, d1, buf)
        buf[n // 2, 3] -= 1.0
        solve(M1, d1, buf); cho(M1, d1, buf)                                        # noqa: E702
        buf[0, 0] += 1.0
        d1.check(Z=buf, B=buf)
        cho(M1, d1, buf); gram(M1, d1, buf)                                         # noqa: E702
    finally:
        M1.free()
        M2.free()


CONSUMERS = ("forward_gram", "forward_solve", "cho_solve", "tri_multiply", "predict_terms", "predict_var")


def _consume(ctx, M, name, Z, desc=None, X=None):
    if name == "predict_terms":
        return ctx.predict_terms(M, desc, X, X[:3], rhs=Z)
    if name == "predict_var":
        return ctx.predict_var(M, desc, X, X[:3])
    return getattr(ctx, name)(M, Z)


def check_refusals(ctx, desc):
    """Section 5's refusals: ValueError, and the matrix still serves afterwards where it is in a state that serves."""
    n = 40
    d = design(n, "rand", 7)
    Z = operands(n, 3, 31)
    d.check(Z=Z, B=Z, Y=Z)
    X = np.linspace(0.0, 1.0, n)[:, None]
    from gsum_amd._lib import SeriesScale
    series, ref, ratio = SeriesScale.make(0, 3), np.ones(n), np.full(n, 0.5)

    def refused(fn, *a, **kw):
        with pytest.raises(ValueError):
            fn(*a, **kw)

    # every consumer on an unfactored matrix
    M = ctx.upload(d.A)
    try:
        for name in CONSUMERS:
            refused(_consume, ctx, M, name, Z, desc, X)
        for name in ("cho_solve", "tri_multiply"):              # (no columns: no device call, the same refusal)
            refused(getattr(ctx, name), M, Z[:, :0])
        eq(M.to_host(), d.A)
        assert ctx.potrf(M) == 0                                # ... which left it an input
        eq(M.to_host(), d.L)
        # potrf, pstrf or scale_series on a factorised matrix
        refused(ctx.potrf, M)
        refused(ctx.pstrf, M)
        refused(ctx.sqrt_errors, M, Z, None, pivot=True)
        refused(M.scale_series, series, ref, ratio)
        for name in ("cho_solve", "tri_multiply"):              # no columns on a factor: nothing to do, nothing returned
            assert getattr(ctx, name)(M, Z[:, :0]).shape == (n, 0)
            refused(getattr(ctx, name), M, Z[:-1, :0])
        # wrong row count; k = 0 and k = 17 where one device call is meant
        for name in ("forward_gram", "forward_solve", "cho_solve", "tri_multiply"):
            refused(getattr(ctx, name), M, Z[:-1])
        refused(ctx.sqrt_errors, M, Z[:-1], None, pivot=False)
        for name in ("forward_gram", "forward_solve"):
            refused(getattr(ctx, name), M, Z[:, :0])
            refused(getattr(ctx, name), M, operands(n, 17, 32))
        refused(ctx.predict_terms, M, desc, X, X[:3], rhs=operands(n, 17, 32))
        refused(ctx.predict_terms, M, desc, X[:-1], X[:3])
        check_gram(ctx, M, d, Z)                                # the refusals changed nothing
        eq(M.to_host(), d.L)
    finally:
        M.free()
    # every consumer except sqrt_errors(pivot=True) on a pivoted factor
    P = ctx.upload(d.A)
    try:
        info, piv = ctx.pstrf(P)
        assert info == 0 and P.pivoted
        for name in CONSUMERS:
            refused(_consume, ctx, P, name, Z, desc, X)
        for name in ("cho_solve", "tri_multiply"):
            refused(getattr(ctx, name), P, Z[:, :0])
        refused(ctx.sqrt_errors, P, Z, None, pivot=False)
        refused(ctx.potrf, P)
        refused(ctx.pstrf, P)
        refused(P.scale_series, series, ref, ratio)
        E, _ = ctx.sqrt_errors(P, Z, None, pivot=True)          # ... which its one consumer still takes
        assert E.shape == (n, 3) and np.all(np.isfinite(E))
    finally:
        P.free()
    # any call but to_host and free on a matrix whose factorisation returned info > 0
    for how in ("potrf", "pstrf", "sqrt_errors"):
        Abad = failing(d, (n // 2,), twice=True)
        F = ctx.upload(Abad)
        try:
            if how == "potrf":
                assert ctx.potrf(F) == n // 2 + 1
            elif how == "pstrf":
                assert ctx.pstrf(F)[0] >= 1
            else:
                with pytest.raises(np.linalg.LinAlgError):
                    ctx.sqrt_errors(F, Z, None, pivot=False)
            assert F.failed and not F.factored
            for name in CONSUMERS:
                refused(_consume, ctx, F, name, Z, desc, X)
            refused(ctx.potrf, F)
            refused(ctx.pstrf, F)
            refused(ctx.sqrt_errors, F, Z, None, pivot=False)
            refused(ctx.sqrt_errors, F, Z, None, pivot=True)
            refused(F.scale_series, series, ref, ratio)
            for name in ("cho_solve", "tri_multiply"):
                refused(getattr(ctx, name), F, Z[:, :0])
            assert F.to_host().shape == (n, n)
            if how == "pstrf":
                eq(F.to_host(), Abad)                           # a rank-deficient search leaves the entries as they were
        finally:
            F.free()


def check_predict_var_contract(ctx, desc):
    """predict_var(want_vtw=True) on a small kernel-built factor: available after forward_gram, forward_solve and
    predict_terms(rhs=...), refused after cho_solve and on a fresh factor; what it returns is V^T W of the right-hand sides held."""
    n, m = 48, 5
    X = np.linspace(0.0, 1.0, n)[:, None]
    Xs = np.linspace(0.05, 0.95, m)[:, None]
    rng = np.random.default_rng(41)
    z1, z2, z3 = rng.standard_normal((n, 2)), rng.standard_normal((n, 3)), rng.standard_normal((n, 1))
    L, info = ctx.factorize(desc, X, diag_add=1e-6)
    assert info == 0

    def vtw_of(z):
        css, vtw = ctx.predict_var(L, desc, X, Xs, want_vtw=True)
        css0, want, _ = ctx.predict_terms(L, desc, X, Xs, rhs=z)
        assert vtw.shape == (m, GSUM_MAX_RHS)
        np.testing.assert_allclose(vtw[:, :z.shape[1]], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        eq(vtw[:, z.shape[1]:], 0.0)
        np.testing.assert_allclose(css, css0, rtol=1e-12)

    try:
        with pytest.raises(ValueError):
            ctx.predict_var(L, desc, X, Xs, want_vtw=True)      # a fresh factor holds no solve
        css, none = ctx.predict_var(L, desc, X, Xs)             # ... and serves the sums of squares
        assert none is None and css.shape == (m,)
        ctx.forward_gram(L, z1)
        vtw_of(z1)
        ctx.cho_solve(L, z1)
        with pytest.raises(ValueError):
            ctx.predict_var(L, desc, X, Xs, want_vtw=True)      # cho_solve overwrote it
        ctx.forward_solve(L, z2)
        vtw_of(z2)
        ctx.cho_solve(L, z3)
        with pytest.raises(ValueError):
            ctx.predict_var(L, desc, X, Xs, want_vtw=True)
        ctx.predict_terms(L, desc, X, Xs, rhs=z3)
        vtw_of(z3)
        ctx.tri_multiply(L, z1)                                 # leaves the held solve alone
        vtw_of(z3)
    finally:
        L.free()
