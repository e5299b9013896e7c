"""Designs that put all three classes of the kernel build's exp argument into its tiles, with their host-side truth (no tests here).

Every entry of a kernel matrix takes the exponential of an argument x (gsum_amd/csrc/kernels/build.hip.h, header comment: u = X / length_scale,
s = sum_m (u_im - u_jm)^2 summed in feature order; RBF x = -s / 2; Matern d = sqrt(s), t = d sqrt(3) or d sqrt(5), x = -t; Matern 1/2 x = -d)
and x falls into one of three classes, which the build treats differently:

    IN_RANGE   |x| < 707.7 (0x1.61da04cbafe44p+9)     numpy's table algorithm restated (gs_exp_core, behind gs_exp_np, gs_exp_np_t, gs_exp_np_nobranch)
    BAND       -745.2 <= x <= -707.7                  the result is subnormal (or rounds to zero: exp(x) = 0 from x < -745.1332): the device
                                                      library's exp; in full off-diagonal ("plain") tiles after a wave-wide ballot
    FAR        x < -745.2                             exactly 0.0; a two-row x 128-column group that is far throughout skips the arithmetic

``Design`` holds a kernel, X and Y; ``Design.entries()`` / ``entries(cross=True)`` give, for kern(X) / kern(X, Y), every leaf's argument,
the entry's class, the polynomial factor p (1 for RBF and Matern 1/2, 1 + t for Matern 3/2, 1 + t + t^2 / 3 for Matern 5/2) and the
``numpy.longdouble`` truth  sum over leaves of weight p exp(x) (+ constants; the one-argument form's diagonal: leaves forced to 1, white
noise on).  A kernel with several stationary leaves (RBF + RBF) has several arguments per entry; the entry is BAND if any leaf is, else FAR
if every leaf is, else IN_RANGE (in-range leaves plus exact zeros).

The bound on an entry K against a reference ``want`` (scikit-learn's matrix on the device; the truth for scikit-learn itself):
    FAR        K == far_value exactly (amplitude * 0.0 + additive_const, in scikit-learn's order of operations)
    IN_RANGE   |K - want| <= 4 spacing(max(|K|, |want|))                       (tests/test_gpu_parity.py's kernel-entry tolerance)
    BAND       |K - want| <= 4 spacing(max(|K|, |want|)) + 4 sub_scale,        sub_scale = 5e-324 sum over the band leaves of weight p
the second term being four subnormal spacings of the exponential carried through the factor that multiplies it.

Tile geometry restated for the coverage counts (``group_counts``): k_build2 works on 32-row slices x 128-column tiles, a wave on the row
pairs (2 q, 2 q + 1) and all 128 columns at once; gs_build_tile128 (inside k_lml_medium, lower tiles only) on 128 x 128 tiles with row
pairs (r, r + 4), r mod 8 < 4.  A tile is plain when it is complete and off the diagonal; the two ballots exist only there.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

LD = np.longdouble
IN_RANGE, BAND, FAR = 0, 1, 2
CLASS_NAMES = ("in range", "band", "far")
IN_RANGE_LIMIT = float.fromhex("0x1.61da04cbafe44p+9")       # 707.7...: GS_EXP_INRANGE, the table algorithm's limit
FAR_LIMIT = -745.2                                          # gs_exp_np_nobranch's far threshold
SUBNORMAL = 5e-324
ULPS = 4
NUGGET = 1e-8                                               # of the likelihood runs (test_medium_fused_path_matches_general_path's)
SQRT3, SQRT5 = 1.7320508075688772, 2.23606797749979         # math.sqrt(3), math.sqrt(5): scikit-learn's own constants


def _ns():
    from sklearn.gaussian_process.kernels import RBF, Matern, WhiteKernel, ConstantKernel as C
    return dict(RBF=RBF, Matern=Matern, WhiteKernel=WhiteKernel, C=C, np=np)


def _leaves(k, weight=1.0):
    """[(stationary leaf, product of the constants that multiply it)] of a sum of products."""
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Product, Sum, WhiteKernel
    if isinstance(k, Sum):
        return _leaves(k.k1, weight) + _leaves(k.k2, weight)
    if isinstance(k, Product):
        factors, consts = [], weight
        for f in (k.k1, k.k2):
            if isinstance(f, ConstantKernel):
                consts *= f.constant_value
            else:
                factors.append(f)
        return sum((_leaves(f, consts) for f in factors), [])
    if isinstance(k, (WhiteKernel, ConstantKernel)):
        return []
    assert isinstance(k, RBF), k                              # (Matern subclasses RBF)
    return [(k, weight)]


def _with_leaves(k, leaf, white):
    """The kernel's value with every stationary leaf replaced by ``leaf`` and every WhiteKernel by ``white``, in scikit-learn's order of
    operations (Sum: k1 + k2, Product: k1 * k2)."""
    from sklearn.gaussian_process.kernels import ConstantKernel, Product, Sum, WhiteKernel
    if isinstance(k, Sum):
        return _with_leaves(k.k1, leaf, white) + _with_leaves(k.k2, leaf, white)
    if isinstance(k, Product):
        return _with_leaves(k.k1, leaf, white) * _with_leaves(k.k2, leaf, white)
    if isinstance(k, ConstantKernel):
        return type(leaf)(k.constant_value)
    if isinstance(k, WhiteKernel):
        return type(leaf)(k.noise_level) if white else type(leaf)(0.0)
    return leaf


@dataclass
class Entries:
    args: list              # per leaf: the exp argument of every entry (float64)
    cls: np.ndarray         # IN_RANGE / BAND / FAR per entry
    p: list                 # per leaf: the polynomial factor (float64)
    sub_scale: np.ndarray   # 5e-324 * sum over the band leaves of weight * p
    truth: np.ndarray       # longdouble
    far_value: float
    diag: np.ndarray        # bool: the one-argument form's diagonal (all False for the cross form)

    def counts(self):
        off = ~self.diag
        return tuple(int(np.sum((self.cls == c) & off)) for c in (IN_RANGE, BAND, FAR))

    def bound(self, K, want):
        """The entrywise bound of the module docstring on |K - want| (FAR entries: 0)."""
        K, want = np.asarray(K, dtype=np.float64), np.asarray(want, dtype=np.float64)
        b = ULPS * np.spacing(np.maximum(np.abs(K), np.abs(want)))
        b = b + np.where(self.cls == BAND, ULPS * self.sub_scale, 0.0)
        return np.where(self.cls == FAR, 0.0, b)


@dataclass(frozen=True)
class Design:
    name: str
    expr: str               # the kernel over RBF, Matern, WhiteKernel, C and np
    n: int
    step: float             # feature 0 is step * arange(n)
    d: int = 1
    m: int = 300            # rows of Y (feature 0: the same grid, a quarter step to the side: no coincident points)
    shuffle: bool = False   # rows of X permuted by a fixed seed: no diagonal structure, single lanes of every class in one wave
    tree: bool = False      # walked as a postfix program on the device (gs_tree_eval), also where the flattened descriptor would cover it
    truth_lml: bool = False  # one design per family also goes against the long-double Cholesky (RBF: the one with white noise -- the
    #                          bare RBF grid, four points per length scale, has cond_2 = 1e9 under the nugget)

    @property
    def kernel(self):
        return eval(self.expr, {"__builtins__": {}}, _ns())

    def inputs(self):
        """X (n, d), Y (m, d), Z (n, 6) = [randn | 1].  Features beyond the first: a small periodic offset, another period per feature."""
        n, d, m = self.n, self.d, self.m
        X = np.zeros((n, d))
        X[:, 0] = self.step * np.arange(n)
        for f in range(1, d):
            X[:, f] = 0.01 * f * (np.arange(n) % (f + 2))
        Y = X[:m].copy()
        Y[:, 0] += 0.25 * self.step
        if d > 1:
            Y[:, 1:] = Y[::-1, 1:]
        rng = np.random.RandomState(zlib.crc32(self.name.encode()) & 0x7FFFFFFF)
        if self.shuffle:
            X = X[rng.permutation(n)]
        Z = np.concatenate([rng.randn(n, 5), np.ones((n, 1))], axis=1)
        for a in (X, Y, Z):
            a.setflags(write=False)
        return X, Y, Z

    def describe(self, kernel=None):
        """The device descriptor (of ``kernel``: this design's at another theta): ``describe_kernel``'s, or the postfix program where
        ``tree`` asks for the walk."""
        import gsum_amd
        from gsum_amd import kernels as gk
        kern = self.kernel if kernel is None else kernel
        desc = gsum_amd.describe_kernel(kern, self.d)
        if self.tree and not desc.is_tree:
            desc = gk._describe_tree(gk._compile_tree(kern)[0], None, self.d, kern)
        assert desc.is_tree == self.tree, self.name
        return desc

    def entries(self, cross=False) -> Entries:
        key = (self.name, cross)
        if key not in _ENTRIES:
            _ENTRIES[key] = self._entries(cross)
        return _ENTRIES[key]

    def _entries(self, cross):
        from sklearn.gaussian_process.kernels import Matern
        X, Y, _ = self.inputs()
        kern = self.kernel
        B = Y if cross else X
        diag = np.zeros((len(X), len(B)), dtype=bool)
        if not cross:
            np.fill_diagonal(diag, True)
        args, ps, leaf_cls, weights = [], [], [], []
        truth = None
        for leaf, weight in _leaves(kern):
            ls = np.broadcast_to(np.asarray(leaf.length_scale, dtype=float), (self.d,))
            ua, ub = X / ls, B / ls                                       # divide first, like pdist / cdist on the scaled points
            s = np.zeros((len(X), len(B)))
            for f in range(self.d):
                e = ua[:, f][:, None] - ub[:, f][None, :]
                s = s + e * e
            nu = float(leaf.nu) if isinstance(leaf, Matern) else None
            if nu is None:
                x, p = -0.5 * s, np.ones_like(s)
            else:
                dist = np.sqrt(s)
                if nu == 0.5:
                    x, p = -dist, np.ones_like(s)
                elif nu == 1.5:
                    t = dist * SQRT3
                    x, p = -t, 1.0 + t
                else:
                    assert nu == 2.5
                    t = dist * SQRT5
                    x, p = -t, 1.0 + t + (t * t) / 3.0
            c = np.where(x < FAR_LIMIT, FAR, np.where(np.abs(x) < IN_RANGE_LIMIT, IN_RANGE, BAND))
            value = p.astype(LD) * np.exp(x.astype(LD))
            value[diag] = 1
            term = LD(weight) * value
            truth = term if truth is None else truth + term
            args.append(x), ps.append(p), leaf_cls.append(c), weights.append(weight)
        lc = np.array(leaf_cls)
        cls = np.where((lc == BAND).any(axis=0), BAND, np.where((lc == FAR).all(axis=0), FAR, IN_RANGE))
        cls[diag] = IN_RANGE
        sub = np.zeros(cls.shape)
        for c, p, w in zip(leaf_cls, ps, weights):
            sub = sub + np.where(c == BAND, abs(w) * p * SUBNORMAL, 0.0)
        # constants and white noise: the whole kernel with the leaves at zero is what is added to the leaves' terms
        const_off = _with_leaves(kern, LD(0), white=False)
        const_diag = _with_leaves(kern, LD(0), white=True)
        truth = truth + np.where(diag, const_diag, const_off)
        return Entries(args=args, cls=cls, p=ps, sub_scale=sub, truth=truth, far_value=float(_with_leaves(kern, 0.0, white=False)),
                       diag=diag)

    def sklearn(self, cross=False):
        key = (self.name, cross)
        if key not in _SKLEARN:
            X, Y, _ = self.inputs()
            K = self.kernel(X, Y) if cross else self.kernel(X)
            K.setflags(write=False)
            _SKLEARN[key] = K
        return _SKLEARN[key]


_ENTRIES, _SKLEARN = {}, {}

_LS8 = "[0.3, 0.9, 1.4, 0.7, 1.1, 0.8, 1.6, 1.2]"
DESIGNS = [
    # ---- one-dimensional flat designs: every family on a uniform grid
    Design("rbf", "RBF(0.2)", 400, 0.05),
    Design("matern52", "Matern(0.3, nu=2.5)", 640, 0.3, truth_lml=True),
    Design("matern32", "Matern(0.4, nu=1.5)", 640, 0.5, truth_lml=True),
    Design("matern12", "Matern(0.8, nu=0.5)", 640, 1.9, truth_lml=True),
    # ---- descriptor fields: amp * 0.0 + addc of a skipped group and amp * b + addc of a recomputed lane become visible
    Design("rbf_amplitude_white", "C(1.7) * RBF(0.2) + WhiteKernel(1e-3, noise_level_bounds='fixed')", 400, 0.05, truth_lml=True),
    Design("matern32_additive", "Matern(0.4, nu=1.5) + C(0.5, constant_value_bounds='fixed')", 640, 0.5),
    # ---- anisotropic (the D1 = false instantiations): the grid in feature 0, small periodic offsets in the others
    Design("rbf_2d", "RBF([0.2, 0.7])", 400, 0.05, d=2),
    Design("matern52_8d", f"Matern({_LS8}, nu=2.5)", 640, 0.3, d=8),
    # ---- ragged: n mod 32 and n mod 128 are not zero, Y is not square: edge tiles take the non-plain branch, interior tiles stay plain
    Design("rbf_ragged", "RBF(0.2)", 421, 0.05),
    Design("matern52_ragged", "C(0.6) * Matern(0.3, nu=2.5)", 613, 0.3, m=333),
    # ---- shuffled rows: far, band and in-range lanes mixed inside one wave
    Design("rbf_shuffled", "RBF(0.2)", 400, 0.05, shuffle=True),
    # ---- trees: the branchy exp through gs_tree_eval
    Design("tree_rbf_rbf", "RBF(0.2) + RBF(0.5)", 640, 0.05, tree=True),
    Design("tree_matern52", "C(1.3) * Matern(0.3, nu=2.5) + WhiteKernel(1e-6)", 640, 0.3, tree=True),
]
DESIGN_IDS = [d.name for d in DESIGNS]


# ---- tile geometry -----------------------------------------------------------------------------------------------------------------
def _group_stats(cls, plain_tiles, tile_rows, pair_rows):
    """Row-pair groups (2 rows x 128 columns) of the plain tiles: how many are far throughout, how many hold a band lane and a far lane,
    how many hold all three classes.  ``plain_tiles``: (first row, first column); ``pair_rows``: the pairs' row offsets within a tile."""
    all_far = band_far = all_three = groups = 0
    for r0, c0 in plain_tiles:
        t = cls[r0:r0 + tile_rows, c0:c0 + 128]
        for a, b in pair_rows:
            g = t[[a, b]]
            has = [bool((g == c).any()) for c in (IN_RANGE, BAND, FAR)]
            groups += 1
            all_far += has[2] and not has[0] and not has[1]
            band_far += has[1] and has[2]
            all_three += all(has)
    return dict(groups=groups, all_far=all_far, band_and_far=band_far, all_three=all_three)


def group_counts(design: Design):
    """Per tile geometry, the counts of ``_group_stats``: k_build2 on kern(X) (lower plain tiles: what the lower-only build runs and a
    subset of the full one), k_build2<CROSS> on kern(X, Y), gs_build_tile128 on kern(X) (k_lml_medium: lower tiles)."""
    n, m = design.n, design.m
    one, cross = design.entries().cls, design.entries(cross=True).cls
    pairs32 = [(2 * q, 2 * q + 1) for q in range(16)]
    pairs128 = [(r, r + 4) for r in range(128) if r % 8 < 4]
    lower32 = [(r0, c0) for r0 in range(0, n - 31, 32) for c0 in range(0, n - 127, 128) if c0 + 128 <= r0]
    cross32 = [(r0, c0) for r0 in range(0, n - 31, 32) for c0 in range(0, m - 127, 128)]
    lower128 = [(r0, c0) for r0 in range(0, n - 127, 128) for c0 in range(0, r0, 128)]
    return {"k_build2": _group_stats(one, lower32, 32, pairs32),
            "k_build2_cross": _group_stats(cross, cross32, 32, pairs32),
            "gs_build_tile128": _group_stats(one, lower128, 128, pairs128)}


# ---- the closed form ---------------------------------------------------------------------------------------------------------------
CLOSED_FORM_NS = (384, 421)
CLOSED_FORM_STEP = 8.0           # RBF(0.2) on 8 arange(n): the nearest neighbours' argument is -800, every off-diagonal entry is FAR
