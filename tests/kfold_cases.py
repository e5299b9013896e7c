"""Inputs, truths and the checks that both backends run, shared by test_kfold_cpu.py and test_gpu_kfold.py (no tests here).

Fold layouts, each for an edge of the device kernels (blocks of 128 rows, product tiles of 64, MFMA fragments of 16):

    blocks5        five contiguous blocks: at n = 129 and 257 they straddle the 128-row block boundary of W
    interleaved3   i mod 3: every group touches every block of W, the worst case for the skipped zeros of the Gram product
    random_sizes   a seeded random partition with the sizes 1, 15, 16, 17, 63, 64, 65 as far as n holds them, and the rest (17 points
                   at n = 129, 16 at 257, 400 at 641: more than one block of the group's own factorisation)
    one_group      everything in one group
    singletons     n groups of one point

The truth of a case is a brute force in numpy.longdouble from the SAME float64 factor L the code under test gets: K = L L^T, and
for every group its rows and columns deleted, the rest factored with loo_cases.cholesky_ld and conditioned on.
"""
import functools

import numpy as np

import loo_cases as lc

FLOOR = lc.FLOOR
TRUTH_SIZES = (129, 257)
TRUTH_LAYOUTS = ("blocks5", "interleaved3", "random_sizes", "one_group")
LAYOUTS = TRUTH_LAYOUTS + ("singletons",)
EDGE_SIZES = (1, 15, 16, 17, 63, 64, 65)


def layout(name, n):
    """The groups of a layout at size n: a list of int64 index arrays that partition 0 .. n - 1."""
    idx = np.arange(n, dtype=np.int64)
    if name == "blocks5":
        return [a for a in np.array_split(idx, 5)]
    if name == "interleaved3":
        return [idx[q::3] for q in range(3)]
    if name == "random_sizes":
        perm = np.random.RandomState(7).permutation(n).astype(np.int64)
        groups, at = [], 0
        for s in EDGE_SIZES:
            if at + s >= n:
                break
            groups.append(perm[at:at + s])
            at += s
        groups.append(perm[at:])
        return groups
    if name == "one_group":
        return [idx]
    if name == "singletons":
        return [idx[i:i + 1] for i in range(n)]
    raise ValueError(name)


def labels_of(groups, n):
    lab = np.empty(n, dtype=np.int64)
    for q, g in enumerate(groups):
        lab[g] = q
    return lab


# -- exact plumbing ----------------------------------------------------------------------------------------------------------
def diagonal_case(n, k=3, seed=11):
    """(L, Y, exps): L = diag(2^e_i) with e_i in {1, 2, 3} at 48 random points (all of them where n < 48) and 0 elsewhere, Y of small
    integers.  Then resid = y, var_i = 4^e_i and md2 = sum y_i^2 4^-e_i are exact in fp64 in any order, and log det = 2 ln 2 sum
    e_i is a sum of at most 48 nonzero terms of one sign, each an integer multiple of the rounded ln 2: its rounding error is at
    most (48 + 2) 2^-53 of its value whatever the order, inside FLOOR = 64 * 2^-53."""
    rs = np.random.RandomState(seed)
    exps = np.zeros(n, dtype=np.int64)
    at = rs.permutation(n)[:48]
    exps[at] = rs.randint(1, 4, size=at.size)
    Y = rs.randint(-4, 5, size=(n, k)).astype(float)
    return np.diag(2.0 ** exps), Y, exps


def diagonal_truth(groups, Y, exps):
    """(var (n,), md2 (n_folds, k), logdet (n_folds,)) of diagonal_case, exactly."""
    var = 4.0 ** exps
    md2 = np.stack([(Y[g] ** 2 / var[g][:, None]).sum(0) for g in groups])
    logdet = np.array([2.0 * np.log(2.0) * exps[g].sum() for g in groups])
    return var, md2, logdet


# -- long-double brute force -------------------------------------------------------------------------------------------------
def _forward_ld(L, B):
    """L^-1 B in long double by forward substitution (L lower triangular, B (m, c))."""
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def brute_force_ld(L, R, groups):
    """(resid (n, k), var (n,), md2 (n_folds, k), logdet (n_folds,)) in numpy.longdouble: every group predicted from the others under
    N(0, L L^T), by deleting the group's rows and columns, factoring the rest and conditioning."""
    Ll = np.tril(np.asarray(L)).astype(np.longdouble)
    K = Ll @ Ll.T
    R = np.asarray(R).astype(np.longdouble)
    n, k = R.shape
    resid = np.zeros((n, k), dtype=np.longdouble)
    var = np.zeros(n, dtype=np.longdouble)
    md2 = np.zeros((len(groups), k), dtype=np.longdouble)
    logdet = np.zeros(len(groups), dtype=np.longdouble)
    for q, G in enumerate(groups):
        G = np.sort(G)
        rest = np.setdiff1d(np.arange(n), G)
        cov, e = K[np.ix_(G, G)], R[G]
        if rest.size:
            Lr = lc.cholesky_ld(K[np.ix_(rest, rest)])
            S = _forward_ld(Lr, K[np.ix_(rest, G)])
            cov = cov - S.T @ S
            e = e - S.T @ _forward_ld(Lr, R[rest])
        Lc = lc.cholesky_ld(cov)
        z = _forward_ld(Lc, e)
        resid[G], var[G] = e, np.diag(cov)
        md2[q] = (z * z).sum(0)
        logdet[q] = 2 * np.sum(np.log(np.diag(Lc)))
    return resid, var, md2, logdet


@functools.lru_cache(maxsize=None)
def truth_case(name, n, lay):
    """(L, R, groups, truth) of a class of loo_cases at size n under a layout; truth = brute_force_ld(L, R, groups), read-only."""
    L, R, _, _ = lc.factor_case(name, n)
    groups = layout(lay, n)
    truth = brute_force_ld(L, R, groups)
    for arr in truth:
        arr.setflags(write=False)
    return L, R, groups, truth


def distances(got, truth):
    """The distances of (resid, var, md2, logdet) from the truth: resid and md2 relative to the truth's largest entry, var relative
    per entry, logdet relative to max(1, |truth|)."""
    ld = np.longdouble
    resid, var, md2, logdet = (np.asarray(a).astype(ld) for a in got)
    t_resid, t_var, t_md2, t_logdet = truth
    return {
        "resid": float(np.max(np.abs(resid - t_resid)) / np.max(np.abs(t_resid))),
        "var": float(np.max(np.abs(var - t_var) / t_var)),
        "md2": float(np.max(np.abs(md2 - t_md2)) / np.max(np.abs(t_md2))),
        "logdet": float(np.max(np.abs(logdet - t_logdet) / np.maximum(1, np.abs(t_logdet)))),
    }


def raw_folds(f, groups, R):
    """(resid, var, md2, logdet) of a LooFactor as its backend returns them (no FoldResult arithmetic on top)."""
    return f._raw_folds(groups, R)[2]


# -- checks that run on both backends (called by the tests of both files) ----------------------------------------------------
def check_precision_block_lattice(kind, n, backend):
    """precision_block of an exact lattice against its integer closed form, bit for bit: contiguous, strided and unsorted index
    lists, and lists that reach into the last, partly padded block."""
    from gsum_amd.loo import LooFactor
    L, _, _ = lc.lattice(kind, n)
    i, j = np.indices((n, n))
    if kind == "subdiag":
        P = (1 - 2 * ((i - j) % 2)) * (n - np.maximum(i, j))
    else:
        P = 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
        P[-1, -1] = 1
    P = P.astype(float)
    rs = np.random.RandomState(n)
    lists = [np.arange(n), np.arange(0, n, 3), np.arange(n)[::-1], rs.permutation(n)[:max(1, n // 2)], np.arange(max(0, n - 70), n),
             np.array([n - 1]), np.array([0]), rs.permutation(n)[:min(n, 17)]]
    f = LooFactor(L, backend=backend)
    try:
        for idx in lists:
            np.testing.assert_array_equal(f.precision_block(idx), P[np.ix_(idx, idx)])
    finally:
        f.free()


def check_plumbing(n, lay, backend):
    """diagonal_case under a layout: resid, var and md2 bit for bit, logdet within FLOOR; the same results, in the caller's row
    order, under a permuted group order and permuted indices inside every group."""
    from gsum_amd.loo import LooFactor
    L, Y, exps = diagonal_case(n)
    groups = layout(lay, n)
    var, md2, logdet = diagonal_truth(groups, Y, exps)
    rs = np.random.RandomState(3)
    order = rs.permutation(len(groups))
    shuffled = [rs.permutation(groups[q]) for q in order]
    f = LooFactor(L, backend=backend)
    try:
        for grp, sel in ((groups, np.arange(len(groups))), (shuffled, order)):
            resid, v, m, ld = raw_folds(f, grp, Y)
            np.testing.assert_array_equal(resid, Y)
            np.testing.assert_array_equal(v, var)
            np.testing.assert_array_equal(m, md2[sel])
            assert np.all(np.abs(ld - logdet[sel]) <= FLOOR * np.maximum(1.0, np.abs(logdet[sel]))), np.max(np.abs(ld - logdet[sel]))
        res = f.folds(Y + 2.0, shuffled, mean=2.0)
        np.testing.assert_array_equal(res.mean, np.full_like(Y, 2.0))
        np.testing.assert_array_equal(res.fold_of, labels_of(shuffled, n))
        np.testing.assert_array_equal(res.error, Y / np.sqrt(var)[:, None])
        assert res.md2.shape == res.logpdf.shape == (len(groups), Y.shape[1])
        one = f.folds(Y[:, 1], labels_of(groups, n))
        assert one.mean.shape == one.error.shape == (n,) and one.md2.shape == one.logpdf.shape == (len(groups),)
        np.testing.assert_array_equal(one.md2, md2[:, 1])
    finally:
        f.free()


def _gap(got, want, scale):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / scale))


def closed_form_gaps(name, n, backend):
    """The distances of the two layouts that need no truth from the object's own results, in the norms of `distances`: singletons
    against LooFactor.loo (mean relative to the largest residual, var per entry, error relative to the largest, logpdf relative to
    max(1, |logpdf|)), and the one-group layout against resid = r, var = diag(K), logdet = 2 sum_log_diag and md2 = r^T a."""
    from gsum_amd.loo import LooFactor
    L, R, _, _ = lc.factor_case(name, n)
    f = LooFactor(L, backend=backend)
    try:
        loo = f.loo(R, mean=0.25)
        s = f.folds(R, layout("singletons", n), mean=0.25)
        resid, var, md2, logdet = raw_folds(f, layout("one_group", n), R)
        a = f.solve(R)
        sld = f.sum_log_diag
    finally:
        f.free()
    K = L @ L.T
    rta = np.einsum("ij,ij->j", R, a)
    assert s.md2.shape == (n, R.shape[1]) and s.var.shape == (n,)
    return {
        "single_mean": _gap(s.mean, loo.mean, np.max(np.abs(R - loo.mean))),
        "single_var": _gap(s.var, loo.var, loo.var),
        "single_error": _gap(s.error, loo.error, np.max(np.abs(loo.error))),
        "single_logpdf": _gap(s.logpdf, loo.logpdf, np.maximum(1.0, np.abs(loo.logpdf))),
        "single_md2": _gap(s.md2, loo.error ** 2, np.max(loo.error ** 2)),
        "one_resid": _gap(resid, R, np.max(np.abs(R))),
        "one_var": _gap(var, np.diag(K), np.diag(K)),
        "one_logdet": _gap(logdet, 2 * sld, max(1.0, abs(2 * sld))),
        "one_md2": _gap(md2[0], rta, np.max(np.abs(rta))),
    }


def check_independence(n, backend):
    """A group's outputs are bit-identical in two partitions that share it (the rest split in two and in three), with one curve and
    with three, and across two successive calls."""
    from gsum_amd.loo import LooFactor
    L = lc.factor_case("matern52", 641)[0][:n, :n]                  # a leading block of a factor is a factor
    R = lc.curves(n, 3, seed=6)
    perm = np.random.RandomState(5).permutation(n)
    shared, rest = perm[:min(70, n // 2)], perm[min(70, n // 2):]
    two = [shared] + [a for a in np.array_split(rest, 2)]
    three = [a for a in np.array_split(rest, 3)]
    three.insert(2, shared[::-1])                                   # another place in the call, another order of its indices
    f = LooFactor(L, backend=backend)
    try:
        a = raw_folds(f, two, R)
        b = raw_folds(f, three, R)
        np.testing.assert_array_equal(a[0][shared], b[0][shared])
        np.testing.assert_array_equal(a[1][shared], b[1][shared])
        np.testing.assert_array_equal(a[2][0], b[2][2])
        assert a[3][0] == b[3][2]
        for got, want in zip(raw_folds(f, two, R), a):              # a second call
            np.testing.assert_array_equal(got, want)
        c = raw_folds(f, two, R[:, 1:2])                            # one curve of the three
        np.testing.assert_array_equal(c[0][:, 0], a[0][:, 1])
        np.testing.assert_array_equal(c[1], a[1])
        np.testing.assert_array_equal(c[2][:, 0], a[2][:, 1])
        np.testing.assert_array_equal(c[3], a[3])
    finally:
        f.free()
    return two, a
