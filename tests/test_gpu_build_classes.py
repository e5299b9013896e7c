"""The kernel build's three classes of exp argument on every device path (run with ``-m gpu`` on an MI355X): in range (the restated
table algorithm), the subnormal band (the device library's exp, in plain tiles after a wave-wide ballot) and far (exactly zero; a
two-row x 128-column group that is far throughout skips the arithmetic after another ballot).  tests/build_classes.py holds the designs,
their classes and long-double truth and the entrywise bound; tests/test_build_classes_cpu.py shows without a device that every design has
the classes where the ballots decide and that scikit-learn's matrix -- the reference here -- is within the bound of the truth.

Tolerances.  Far entries: exactly amplitude * 0.0 + additive_const.  In-range entries: tests/test_gpu_parity.py's rule (bit-identical where
the host's numpy runs the algorithm the device restates, 4 ulp otherwise).  Band entries: 4 ulp + 4 subnormal spacings of the exponential
times the factor that multiplies it (amplitude * p): the device library's exp and numpy's scalar path may round a subnormal differently.
Diagonal, symmetry and the device forms among themselves: exact.  The fused medium path against the general path: bit-identical.  G and
sum log L_ii against a long-double Cholesky of scikit-learn's matrix: 1e-10 relative.  What was achieved goes to the parity record."""
import numpy as np
import pytest

from conftest import record_parity

pytestmark = pytest.mark.gpu

import gsum_amd  # noqa: E402

import build_classes as bc  # noqa: E402
import grad_truth as gt  # noqa: E402

try:
    from numpy._core._multiarray_umath import __cpu_features__ as _feats
    SVML_HOST = bool(_feats.get("AVX512_SKX"))
except Exception:
    SVML_HOST = False

EPS = float(np.finfo(np.float64).eps)
DIAG_ADD = 1e-10


@pytest.fixture(scope="module")
def ctx():
    return gsum_amd.default_context(0)


@pytest.fixture(scope="module")
def lab():
    """The lab build (libgsum_hip_lab.so): ``build_lower_only`` is not part of the product ABI."""
    return gsum_amd.lab_context(0)


def _where(mask, E, K, want, tile_rows):
    """The first entry of ``mask`` for a failure message: row, column, class, every leaf's argument, both values, its tile."""
    i, j = (int(v[0]) for v in np.nonzero(mask))
    return (f"{int(mask.sum())} entries; first: row {i}, column {j}, class {bc.CLASS_NAMES[E.cls[i, j]]}, exp argument(s) "
            f"{[float(a[i, j]) for a in E.args]}, device {K[i, j]!r}, scikit-learn {want[i, j]!r}, {tile_rows}-row slice {i // tile_rows}, "
            f"128-column tile {j // 128}, row in slice {i % tile_rows}, lane {(j % 128) // 2}")


def check_classes(label, E: bc.Entries, K, want, tile_rows=32):
    """One device matrix against scikit-learn's, class by class (module docstring); records the worst band error in units of
    amplitude * p * 5e-324 (where that term governs) and as a fraction of the bound."""
    assert K.shape == want.shape == E.cls.shape
    far, inr, band = (E.cls == c for c in (bc.FAR, bc.IN_RANGE, bc.BAND))
    off = ~E.diag
    # far: exactly amp * 0.0 + addc, and scikit-learn has the same value there -- no non-zero exponential on either side
    bad = far & (K != E.far_value)
    assert not bad.any(), f"{label}: far entries that are not {E.far_value!r}: " + _where(bad, E, K, want, tile_rows)
    np.testing.assert_array_equal(K[far], E.far_value)
    np.testing.assert_array_equal(want[far], E.far_value)
    # in range: the existing rule of test_kernel_matrix_matches_sklearn
    err = np.abs(K - want)
    bad = inr & off & ~(err <= bc.ULPS * np.spacing(np.maximum(np.abs(K), np.abs(want))))
    assert not bad.any(), f"{label}: in-range entries beyond {bc.ULPS} ulp: " + _where(bad, E, K, want, tile_rows)
    if SVML_HOST:
        bad = inr & off & (K != want)
        assert not bad.any(), f"{label}: in-range entries that are not bit-identical: " + _where(bad, E, K, want, tile_rows)
        np.testing.assert_array_equal(K[inr & off], want[inr & off])
    # band
    bound = E.bound(K, want)
    governs = band & (E.sub_scale >= np.spacing(np.maximum(np.abs(K), np.abs(want))))
    record_parity(f"build_classes/{label}", band_entries=int(band.sum()),
                  worst_band_error_over_bound=float(np.max(err[band] / bound[band])),
                  worst_band_error_in_subnormal_units=float(np.max(err[governs] / E.sub_scale[governs])) if governs.any() else 0.0,
                  band_entries_not_bit_identical=int(np.sum(band & (K != want))),
                  band_zero_pattern_differs=int(np.sum(band & ((K == E.far_value) != (want == E.far_value)))),
                  in_range_entries_not_bit_identical=int(np.sum(inr & off & (K != want))))
    bad = band & ~(err <= bound)
    assert not bad.any(), f"{label}: band entries beyond 4 ulp + 4 subnormal spacings x amplitude x p: " + _where(bad, E, K, want, tile_rows)


def _same_bits(label, A, B, E):
    bad = A != B
    assert not bad.any(), (f"{label}: {int(bad.sum())} entries differ, per class (in range, band, far): "
                           f"{[int(np.sum(bad & (E.cls == c))) for c in (bc.IN_RANGE, bc.BAND, bc.FAR)]}; first at {np.argwhere(bad)[0]}")
    np.testing.assert_array_equal(A, B)


@pytest.mark.parametrize("design", bc.DESIGNS, ids=bc.DESIGN_IDS)
def test_matrices_class_by_class(ctx, lab, design):
    """Step 1: kern(X) through gsum_kernel_build (full form), kern(X, Y) (k_build2<CROSS> / k_build_tree<true>), the device-resident
    lower-only build mirrored on export, and the lab context with build_lower_only 1 and 0 -- each against scikit-learn class by class;
    the diagonal exact, the matrix symmetric, and the four forms of kern(X) bit-identical to each other in all three classes."""
    X, Y, _ = design.inputs()
    desc = design.describe()
    E, Ec = design.entries(), design.entries(cross=True)
    want, wantc = design.sklearn(), design.sklearn(cross=True)
    K = ctx.kernel_matrix(desc, X)
    check_classes(f"{design.name}/host", E, K, want)
    np.testing.assert_array_equal(np.diag(K), np.diag(want))
    np.testing.assert_array_equal(K, K.T)
    Kc = ctx.kernel_matrix(desc, X, Y)
    check_classes(f"{design.name}/cross", Ec, Kc, wantc)
    Kd = ctx.kernel_matrix(desc, X, diag_add=DIAG_ADD)
    np.testing.assert_array_equal(np.diag(Kd), np.diag(want) + DIAG_ADD)
    _same_bits(f"{design.name}: diag_add moves entries off the diagonal", Kd[~E.diag], K[~E.diag], _OffDiagonal(E))
    forms = {}
    M = ctx.kernel_matrix_dev(desc, X, diag_add=DIAG_ADD)
    forms["dev"] = M.to_host()
    M.free()
    try:
        for lower in (1, 0):
            lab.set_option("build_lower_only", lower)
            M = lab.kernel_matrix_dev(desc, X, diag_add=DIAG_ADD)
            forms[f"lab_lower{lower}"] = M.to_host()
            M.free()
    finally:
        lab.set_option("build_lower_only", 1)
    for name, A in forms.items():
        np.testing.assert_array_equal(np.diag(A), np.diag(want) + DIAG_ADD)
        np.testing.assert_array_equal(A, A.T)
        check_classes(f"{design.name}/{name}", E, np.where(E.diag, K, A), want)
        _same_bits(f"{design.name}: {name} against the host form", A, Kd, E)


class _OffDiagonal:
    """The classes of the off-diagonal entries, flattened like ``A[~E.diag]`` (for ``_same_bits``' per-class message)."""

    def __init__(self, E):
        self.cls = E.cls[~E.diag]


def _truth_G_sld(R, Z):
    """G = W^T W with W = L^-1 Z, sum log L_ii and |W|^T |W| in long double, from the float64 R and Z taken as exact."""
    L = gt.cholesky_ld(R)
    n = len(L)
    W = np.zeros(Z.shape, bc.LD)
    Zl = Z.astype(bc.LD)
    for i in range(n):
        W[i] = (Zl[i] - L[i, :i] @ W[:i]) / L[i, i]
    return W.T @ W, np.log(np.diag(L)).sum(), np.abs(W).T @ np.abs(W)


def _both_paths(ctx, X, Z, descs, nugget):
    """lml_resident on the fused medium path (k_lml_medium: gs_build_tile128) and on the general path (k_build2), options restored."""
    ctx.set_inputs(X, Z)
    try:
        ctx.set_option("medium_min_batch", 1)
        med = ctx.lml_resident(descs, nugget)
        ctx.set_option("medium_path", 0)
        gen = ctx.lml_resident(descs, nugget)
    finally:
        ctx.set_option("medium_path", 1)
        ctx.set_option("medium_min_batch", -1)
        ctx.set_option("release_scratch", 1)
    return med, gen


@pytest.mark.parametrize("design", bc.DESIGNS, ids=bc.DESIGN_IDS)
def test_medium_fused_path_and_truth(ctx, design):
    """Steps 2 and 3.  The design's kernel and two neighbours in theta (the band moves by a few diagonals) through k_lml_medium --
    gs_build_tile128: the two ballots of gs_plain_pair on 128 x 128 tiles with row pairs (r, r + 4) -- and through the general path: G, sum log
    L_ii and info bit-identical, as test_medium_fused_path_matches_general_path asserts on inputs without band or far entries.  One design
    per family then goes against the long-double Cholesky of scikit-learn's matrix (tests/grad_truth.py's): sum log L_ii within 1e-10
    relative, G within 1e-10 of |W|^T |W| entrywise (the magnitude of the terms an entry of G = W^T W sums; on its diagonal that is
    1e-10 relative) -- the matrices are well conditioned (cond < 1e5: 1e-16 cond stays below the 1e-10)."""
    X, _, Z = design.inputs()
    kern = design.kernel
    descs = [design.describe(kern.clone_with_theta(kern.theta + dt)) for dt in (0.0, 0.02, -0.02)]
    med, gen = _both_paths(ctx, X, Z, descs, bc.NUGGET)
    assert np.all(gen[2] == 0), gen[2]
    np.testing.assert_array_equal(med[2], gen[2])
    np.testing.assert_array_equal(med[1], gen[1])
    np.testing.assert_array_equal(med[0], gen[0])
    if not design.truth_lml:
        return
    R = design.sklearn() + bc.NUGGET * np.eye(design.n)
    cond = float(np.linalg.cond(R))
    assert 1e-16 * cond <= 1e-10, cond
    G, sld, S = _truth_G_sld(R, Z)
    e_G = float(np.max(np.abs(med[0][0].astype(bc.LD) - G) / S))
    e_sld = float(abs(bc.LD(med[1][0]) - sld) / abs(sld))
    record_parity(f"build_classes/{design.name}/truth", cond=cond, G_error_over_abs_terms=e_G, sld_rel_error=e_sld, bound=1e-10)
    assert e_G <= 1e-10 and e_sld <= 1e-10, (e_G, e_sld)


@pytest.mark.parametrize("n", bc.CLOSED_FORM_NS)
def test_identity_matrix_in_closed_form(ctx, n):
    """RBF(0.2) on X = 8 arange(n): every off-diagonal entry is far, every row-pair group of every plain tile is skipped, and R is exactly
    c I with c = ((amplitude * 1.0 + white_noise) + additive_const) + nugget formed in that order (the build's diagonal rule).  The
    library's definitions (include/gsum_hip.h: L = chol(R), W = L^-1 RHS, G = W^T W, sld = sum_i log L_ii -- HALF the log-determinant)
    then give  G = Z^T Z / c  and  sld = n log(sqrt(c)) = (n / 2) log c.  Bounds: G within 2 n eps of |Z|^T |Z| / c entrywise (the
    summation bound: n terms, each with the three roundings of two divisions by sqrt(c) and a product); sld within 2 n eps (1 + |sld|):
    L_ii = sqrt(c) (1 + delta), |delta| <= eps / 2, puts delta itself -- not delta log c -- into every term log L_ii, which is the 1, and
    the n-term sum adds n eps |sld|.  Both paths (k_lml_medium and the general one), bit-identical; n = 384 is three complete tiles a
    side, 421 leaves ragged edge tiles."""
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C
    X = bc.CLOSED_FORM_STEP * np.arange(n, dtype=float)[:, None]
    Z = np.concatenate([np.random.RandomState(n).randn(n, 5), np.ones((n, 1))], axis=1)
    kerns = [RBF(0.2), C(1.7) * RBF(0.2) + WhiteKernel(1e-3, noise_level_bounds="fixed")]
    descs = [gsum_amd.describe_kernel(k, 1) for k in kerns]
    med, gen = _both_paths(ctx, X, Z, descs, bc.NUGGET)
    for a, b in zip(med, gen):
        np.testing.assert_array_equal(a, b)
    assert np.all(med[2] == 0)
    Zl = Z.astype(bc.LD)
    for i, desc in enumerate(descs):
        np.testing.assert_array_equal(ctx.kernel_matrix(desc, X, diag_add=bc.NUGGET),
                                      (((desc.amplitude * 1.0 + desc.white_noise) + desc.additive_const) + bc.NUGGET) * np.eye(n))
        c = bc.LD(((desc.amplitude * 1.0 + desc.white_noise) + desc.additive_const) + bc.NUGGET)
        G, S = Zl.T @ Zl / c, np.abs(Zl).T @ np.abs(Zl) / c
        sld = bc.LD(n) * np.log(np.sqrt(c))
        e_G = float(np.max(np.abs(med[0][i].astype(bc.LD) - G) / S))
        e_sld = float(abs(bc.LD(med[1][i]) - sld) / (1 + abs(sld)))
        record_parity(f"build_classes/identity_n{n}_kernel{i}", c=float(c), G_error_in_n_eps=e_G / (n * EPS), sld_error_in_n_eps=e_sld / (n * EPS),
                      bound_in_n_eps=2.0)
        assert e_G <= 2 * n * EPS and e_sld <= 2 * n * EPS, (i, e_G / (n * EPS), e_sld / (n * EPS))
