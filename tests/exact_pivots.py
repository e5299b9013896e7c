"""Inputs on which LAPACK dpstrf's pivot search is exact, and two references for it (no tests here).

A = Q^T blockdiag(B_1, B_2, ...) Q: many copies of a few small blocks B = L0 L0^T, Q a symmetric permutation.  L0 is integer lower
triangular of size b <= 9: its first r rows have diagonal 2^e with strictly decreasing exponents in [2, 10], its last b - r rows a zero
diagonal (rank-deficient blocks), and every off-diagonal entry in a nonzero column is in {-1, 0, 1}.  Inside a block the residual diagonal
of row i once rows 0 .. k-1 are eliminated is 4^e_i + (at most b - 1), and 4^e_j >= 4 * 4^e_i for j < i, so the pivots of a block follow
its natural order strictly and take exactly the values 4^e.  Every quantity the search forms is then an integer or a power of two
(sqrt, 1 / sqrt, the scaled columns, every dot product, in any order of summation), all below 2^53: the search is exact.  The zero rows'
residuals are exactly 0 once their block's nonzero rows are gone, and are below 16 before that, so the rank is the number of nonzero rows.
Copies of a block (and blocks sharing an exponent) tie exactly, so almost every step is a multi-way tie that the current positions decide.

``dense_pstf2`` restates dpstf2 (unblocked, lower, tol < 0) on a dense matrix; ``structured_pstrf`` gets the same pivots, rank and factor
from the block structure in O(n b log n).
"""
from __future__ import annotations

import heapq
from dataclasses import dataclass

import numpy as np

EPS = 2.0 ** -53            # dlamch('Epsilon')
MAX_B = 9
EXPONENTS = range(2, 11)    # pivots 4^2 .. 4^10: |A| <= 2^20 + 8


def make_block(rng, r, z=0):
    """L0 with r nonzero rows (diagonal 2^e, e strictly decreasing in [2, 10]) and z trailing zero-diagonal rows."""
    b = r + z
    assert 1 <= b <= MAX_B and r <= len(EXPONENTS)
    e = np.sort(rng.choice(np.array(EXPONENTS), size=r, replace=False))[::-1]
    L0 = np.zeros((b, b), dtype=np.int64)
    for i in range(b):
        L0[i, :min(i, r)] = rng.integers(-1, 2, size=min(i, r))
        if i < r:
            L0[i, i] = 1 << int(e[i])
    return L0


@dataclass
class Spec:
    """blocks: the distinct L0; mult: copies of each; arrangement: 'sorted' (the blocks one after another in natural row order),
    'reversed' (that order backwards) or 'random' (a random permutation, seeded); rows[t]: (copies, b) A-row indices of each copy's
    local rows."""
    blocks: list
    mult: list
    arrangement: str
    seed: int
    negate: bool = False

    def __post_init__(self):
        self.n = int(sum(m * len(B) for B, m in zip(self.blocks, self.mult)))
        n = self.n
        if self.arrangement == "sorted":
            sigma = np.arange(n)
        elif self.arrangement == "reversed":
            sigma = np.arange(n)[::-1].copy()
        elif self.arrangement == "random":
            sigma = np.random.default_rng(self.seed + 7919).permutation(n)
        else:
            raise ValueError(self.arrangement)
        # sorted row s (blocks one after another) is row a_of_s[s] of A
        a_of_s = np.empty(n, dtype=np.int64)
        a_of_s[sigma] = np.arange(n)
        self.rows, s0 = [], 0
        for B, m in zip(self.blocks, self.mult):
            b = len(B)
            self.rows.append(a_of_s[s0:s0 + m * b].reshape(m, b))
            s0 += m * b
        self.rank = int(sum(m * int(np.count_nonzero(np.diag(B))) for B, m in zip(self.blocks, self.mult)))

    def dense(self):
        """A (n x n float64)."""
        A = np.zeros((self.n, self.n))
        for L0, R in zip(self.blocks, self.rows):
            B = (L0 @ L0.T).astype(float)
            A[R[:, :, None], R[:, None, :]] = -B if self.negate else B
        return A

    def factor_coo(self):
        """blockdiag(L0) in A's row / column indices: (rows, cols, values) of its nonzeros, columns of nonzero pivots only."""
        ri, ci, vs = [], [], []
        for L0, R in zip(self.blocks, self.rows):
            i, j = np.nonzero(L0)
            ri.append(R[:, i].ravel())
            ci.append(R[:, j].ravel())
            vs.append(np.tile(L0[i, j].astype(float), len(R)))
        return np.concatenate(ri), np.concatenate(ci), np.concatenate(vs)


def tie_spec(n, rank=None, arrangement="random", seed=0, types=4):
    """n rows of copies of `types` random blocks (plus 1 x 1 blocks [4^k] / [0] to hit n and the rank exactly)."""
    rank = n if rank is None else rank
    assert 0 <= rank <= n
    rng = np.random.default_rng(seed)
    deficient = rank < n
    kinds = []
    for t in range(types):
        z = int(rng.integers(1, 4)) if deficient and t % 2 == 0 else 0      # (deficient inputs: every other kind has zero rows)
        kinds.append(make_block(rng, int(rng.integers(1, MAX_B - z + 1)), z))
    ones = {k: np.array([[1 << k]], dtype=np.int64) for k in EXPONENTS}
    zero = np.zeros((1, 1), dtype=np.int64)
    counts = {}
    R, D = rank, n - rank
    for _ in range(4 * n):
        t = int(rng.integers(len(kinds)))
        r = int(np.count_nonzero(np.diag(kinds[t])))
        z = len(kinds[t]) - r
        if r <= R and z <= D:
            counts[t] = counts.get(t, 0) + 1
            R, D = R - r, D - z
    blocks, mult = [], []
    for t in sorted(counts):
        blocks.append(kinds[t])
        mult.append(counts[t])
    pads = rng.choice(np.array(EXPONENTS), size=R)
    for k in EXPONENTS:
        c = int(np.count_nonzero(pads == k))
        if c:
            blocks.append(ones[k])
            mult.append(c)
    if D:
        blocks.append(zero)
        mult.append(D)
    spec = Spec(blocks, mult, arrangement, seed)
    assert spec.n == n and spec.rank == rank, (spec.n, spec.rank)
    return spec


def dense_pstf2(A):
    """dpstf2 (lower, tol < 0) restated in float64: (L, piv, rank, info).  L: the factor's first `rank` columns in pivot order (n x n,
    zero beyond); piv 0-based; info 1 when the search stopped early."""
    A = np.array(A, dtype=float)
    n = A.shape[0]
    piv = np.arange(n)
    L = np.zeros((n, n))
    if n == 0:
        return L, piv, 0, 0
    d = np.diag(A).copy()                   # A(I, I) of the row at position I
    work = np.zeros(n)
    pvt = int(np.argmax(d))                 # MAXLOC: the first maximum
    ajj = d[pvt]
    if not ajj > 0.0:                       # AJJ <= 0 or NaN: rank 0
        return L, piv, 0, 1
    dstop = n * EPS * ajj
    for j in range(n):
        if j > 0:
            work[j:] += L[j:, j - 1] ** 2
            cand = d[j:] - work[j:]
            pvt = j + int(np.argmax(cand))
            ajj = cand[pvt - j]
            if ajj <= dstop or np.isnan(ajj):
                return L, piv, j, 1
        if pvt != j:                        # the symmetric swap of rows / columns j and pvt, the dot products and PIV
            A[[j, pvt], :] = A[[pvt, j], :]
            A[:, [j, pvt]] = A[:, [pvt, j]]
            L[[j, pvt], :j] = L[[pvt, j], :j]
            d[[j, pvt]] = d[[pvt, j]]
            work[[j, pvt]] = work[[pvt, j]]
            piv[[j, pvt]] = piv[[pvt, j]]
        ajj = np.sqrt(ajj)
        L[j, j] = ajj
        if j < n - 1:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) * (1.0 / ajj)
    return L, piv, n, 0


@dataclass
class Reference:
    piv: np.ndarray         # (n,) 0-based
    rank: int
    info: int
    rows: np.ndarray        # the factor's nonzeros in pivot order: L[rows, cols] = vals (columns < rank)
    cols: np.ndarray
    vals: np.ndarray

    def dense(self, n):
        L = np.zeros((n, n))
        L[self.rows, self.cols] = self.vals
        return L

    def sparse(self, n):
        from scipy.sparse import csr_matrix
        return csr_matrix((self.vals, (self.rows, self.cols)), shape=(n, n))


def structured_pstrf(spec: Spec, tiebreak="position") -> Reference:
    """dpstrf's pivots, rank and factor on spec's matrix from its block structure.  Each block's candidate is its next natural row, of
    value exactly 4^e and strictly above every other remaining row of the block; a step takes the largest candidate value and, among
    equal ones, the lowest current position (MAXLOC), then swaps positions j and pvt as LAPACK does (the row at j moves to pvt).
    tiebreak='row' takes the lowest A row instead (not LAPACK: it shows that the inputs tell the two apart)."""
    key = (lambda p, a: p) if tiebreak == "position" else (lambda p, a: a)
    n = spec.n
    at = np.arange(n)                       # at[p]: the A row at position p
    pos = np.arange(n)                      # pos[a]: the position of A row a
    owner = np.full(n, -1, dtype=np.int64)  # A row -> block id
    local = np.zeros(n, dtype=np.int64)
    blocks, heap = [], []
    if spec.negate:                         # max diagonal < 0: rank 0 at the first step
        return Reference(at, 0, 1 if n else 0, *(np.zeros(0, dtype=np.int64),) * 2, np.zeros(0))
    for L0, R in zip(spec.blocks, spec.rows):
        dg = np.diag(L0)
        r = int(np.count_nonzero(dg))
        vals = [int(x) * int(x) for x in dg[:r]]
        for rows in R:
            bid = len(blocks)
            blocks.append((rows, vals, r))
            owner[rows] = bid
            local[rows] = np.arange(len(rows))
    nxt = np.zeros(len(blocks), dtype=np.int64)
    for bid, (rows, vals, r) in enumerate(blocks):
        if r:
            heap.append((-vals[0], key(int(pos[rows[0]]), int(rows[0])), int(pos[rows[0]]), int(rows[0])))
    heapq.heapify(heap)

    def is_candidate(a):
        bid = owner[a]
        return nxt[bid] < blocks[bid][2] and local[a] == nxt[bid]

    rank = n
    for j in range(n):
        while heap and (pos[heap[0][3]] != heap[0][2] or not is_candidate(heap[0][3])):
            heapq.heappop(heap)
        if not heap:                        # every remaining residual diagonal is exactly 0 <= dstop
            rank = j
            break
        _, _, p, a = heapq.heappop(heap)
        rt = int(at[j])
        at[j], at[p] = a, rt
        pos[a], pos[rt] = j, p
        if rt != a and is_candidate(rt):
            bid = owner[rt]
            heapq.heappush(heap, (-blocks[bid][1][nxt[bid]], key(p, rt), p, rt))
        bid = owner[a]
        nxt[bid] += 1
        rows, vals, r = blocks[bid]
        if nxt[bid] < r:
            c = int(rows[nxt[bid]])
            heapq.heappush(heap, (-vals[nxt[bid]], key(int(pos[c]), c), int(pos[c]), c))
    ri, ci, vs = spec.factor_coo()
    return Reference(at.astype(np.int64), rank, 0 if rank == n else 1, pos[ri], pos[ci], vs)
