"""The gradient pieces' extended-precision truth (tests/grad_truth.py) and the bound of tests/test_gpu_grad_pieces.py, validated without a
device: the truth is consistent with itself and with a finite difference of log det R; the float64 dense reference (the cpu backend's
``lml_grad``, and a plain cholesky / cho_solve / einsum evaluation) has a normalised error of at most 4 eps on EVERY case of the device
matrix -- so the normalisation removes the conditioning and  e_dev <= 16 max(e_ref, eps)  is a bound of rounding size; and the bound has
teeth: the errors it exists to catch, put into the reference's kernel gradient on the host, exceed it.  Run with -s to see every figure."""
import warnings

import numpy as np
import pytest

import gsum_amd
from gsum_amd._cpu import cpu_context

import grad_truth as gt

EPS = gt.EPS


def test_long_double_is_extended_precision():
    assert np.finfo(np.longdouble).nmant >= 63
    gt._require_extended()


@pytest.mark.parametrize("cid,run", [("small_flat-n17-d1-k5", "tight"), ("small_flat-n17-d1-k5", "amplified"), ("general_flat-n129-d1-k5", "tight"),
                                     ("general_flat-n129-d1-k5", "amplified"), ("general_flat-n257-d2-k5", "amplified")])
def test_truth_inverse_times_matrix_is_the_identity(cid, run):
    case = next(c for c in gt.CASES if c.id == cid)
    n = case.n
    _, _, R, dK, _, _ = case.matrices(dict(gt.RUNS)[run])
    T = gt.pieces_truth(R, dK)
    resid = np.abs(R.astype(gt.LD) @ T.Rinv - np.eye(n, dtype=gt.LD)).max()
    print(f"{case.id}-{run}: cond {T.cond:.3g}  max |R Rinv - I| = {float(resid):.3g} = {float(resid) / T.cond:.3g} cond")
    assert float(resid) <= 1e-15 * T.cond
    # L L^T = R to long-double rounding, and the log-determinant is the factor's
    assert float(np.abs(T.L @ T.L.T - R.astype(gt.LD)).max()) <= 1e-17 * float(np.abs(R).max()) * n
    sign, logdet = np.linalg.slogdet(R)
    assert sign == 1 and abs(2.0 * float(T.sld) - logdet) <= 1e-15 * T.cond * float(T.S_sld)


@pytest.mark.parametrize("path", ["small_flat", "small_tree"])
def test_trace_is_the_derivative_of_log_det(path):
    """trace_p = d log det R / d theta_p: central differences of the long-double log det R at theta +- h and +- h / 2, Richardson-combined
    (truncation O(h^4) ~ 1e-12 at h = 1e-3; R itself is float64 at every theta, which leaves ~ eps n cond / h ~ 1e-10 of S_trace) -- the
    order of the parameters, their signs and the log-parametrisation, for one flattened kernel (d = 8: eleven parameters) and one tree
    (the four-leaf sum: ten)."""
    case = next(c for c in gt.CASES if c.path == path and c.n == 17 and c.d == (8 if path == "small_flat" else 1))
    kern, X, R, dK, _, _ = case.matrices(gt.WHITE_TIGHT)
    T = gt.pieces_truth(R, dK)
    n = case.n

    def logdet(theta):
        Rt = kern.clone_with_theta(theta)(X) + gt.NUGGET * np.eye(n)
        return 2 * np.log(np.diag(gt.cholesky_ld(Rt))).sum()

    h = 1e-3
    assert len(kern.theta) == dK.shape[2] == len(gsum_amd.kernels.describe_gradient(kern, case.d))
    for p in range(len(kern.theta)):
        e = np.zeros(len(kern.theta))
        e[p] = 1.0
        d1 = (logdet(kern.theta + h * e) - logdet(kern.theta - h * e)) / (2 * h)
        d2 = (logdet(kern.theta + h / 2 * e) - logdet(kern.theta - h / 2 * e)) / h
        fd = (4 * d2 - d1) / 3
        err = float(abs(fd - T.trace[p]) / T.S_trace[p])
        print(f"{case.id} theta[{p}]: trace {float(T.trace[p]):+.12e}  finite difference {float(fd):+.12e}  |diff| / S_trace {err:.2e}")
        assert err <= 1e-8


def _reference_errors(case, run, white):
    kern, X, R, dK, Z, Zs, cols, T = gt.case_truth(case, run, white)
    desc, prm = gsum_amd.describe_kernel(kern, case.d), gsum_amd.kernels.describe_gradient(kern, case.d)
    assert len(prm) == dK.shape[2] == len(kern.theta)
    out = {}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")                       # (scikit-learn's own 0 / 0 at coincident points of Matern-1/2)
        for name, rhs in (("random", Z), ("selector", Zs)):
            G, sld, info, tr, H = cpu_context().lml_grad(desc, prm, X, rhs, gt.NUGGET)
            assert info == 0
            out[name, "cpu"] = gt.piece_errors(T, name, G, sld, tr, H)
            out[name, "plain"] = gt.piece_errors(T, name, *gt.reference_pieces(R, dK, rhs))
    return T, out


@pytest.mark.parametrize("case,run,white", gt.CASE_RUNS, ids=gt.CASE_RUN_IDS)
def test_reference_error_of_every_case(case, run, white):
    """e_ref of the float64 dense reference on every case of the device matrix, both runs, both kinds of right-hand sides: finite, info 0,
    at most 4 eps (measured: <= 1.9 eps for H, <= 0.75 eps for the traces over n = 1 ... 513, cond = 1 ... 1.8e8); the tight run's condition
    number is below 1e3."""
    T, out = _reference_errors(case, run, white)
    assert np.isfinite(T.cond) and (run != "tight" or T.cond < 1e3)
    for (name, which), e in out.items():
        print(f"{case.id}-{run} cond {T.cond:.3g} {name:8s} {which:5s} e_ref / eps: "
              + "  ".join(f"{piece} {v / EPS:.3f}" for piece, v in e.items()))
        for piece, v in e.items():
            assert np.isfinite(v) and v <= gt.REF_LIMIT * EPS, (name, which, piece, v / EPS)


def test_entrywise_scale_fails_on_the_selector_and_the_norm_scale_bounds_it():
    """Why the selector's H_p is measured against S_H_norm: under the entrywise S_H the float64 reference itself is ~1e17 eps off (entries of
    H_p whose own dR_p entry is zero carry the solve's error of the whole column), and S_H_norm >= S_H everywhere."""
    case = next(c for c in gt.CASES if c.id == "small_flat-n17-d1-k5")
    kern, X, R, dK, Z, Zs, cols, T = gt.case_truth(case, "tight", gt.WHITE_TIGHT)
    r = T.rhs["selector"]
    H = gt.reference_pieces(R, dK, Zs)[3]
    entrywise = gt.normalised_error(H, r.H, T.cond, r.S_H)
    normwise = gt.normalised_error(H, r.H, T.cond, r.S_H_norm)
    print(f"selector, reference H: entrywise scale {entrywise / EPS:.3g} eps, norm scale {normwise / EPS:.3g} eps")
    assert entrywise > 1e6 * EPS and normwise <= gt.REF_LIMIT * EPS
    for name in ("random", "selector"):
        assert np.all(T.rhs[name].S_H_norm >= T.rhs[name].S_H * (1 - 1e-15))
    # the selector's columns hold what they are there for
    assert cols[0] == case.n - 1 and 0 in cols and np.sum(cols == case.n // 2 + 1) == 2
    dup = next(c for c in gt.CASES if c.dup and c.n == 65)
    Xd, _, cd = dup.inputs()
    assert np.array_equal(Xd[0], Xd[dup.n // 2]) and {0, dup.n // 2} <= set(cd.tolist())


MUTATIONS = ["anisotropic dimension takes the whole distance", "last row skipped", "one parameter scaled by 1 + 1e-9",
             "trace from the lower triangle without the factor 2"]


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_the_bound_catches_the_errors_it_is_for(mutation):
    """The device errors the bound exists for, put into the float64 reference on the host (tight run): each exceeds 16 max(e_ref, eps) in
    the trace or in H_p of at least one kind of right-hand sides."""
    case = next(c for c in gt.CASES if c.id == ("general_flat-n255-d3-k16" if "anisotropic" in mutation or "last" in mutation
                                                else "general_tree-n129-d1-k5"))
    kern, X, R, dK, Z, Zs, cols, T = gt.case_truth(case, "tight", gt.WHITE_TIGHT)
    n = case.n
    bad = dK.copy()
    if "anisotropic" in mutation:
        bad[:, :, 2] = dK[:, :, 1:4].sum(axis=2)             # theta = (amplitude, l_0, l_1, l_2, white, constant): l_1 gets the isotropic sum
    elif "last row" in mutation:
        bad[n - 1, :, :] = 0.0
    elif "scaled" in mutation:
        bad[:, :, 1] *= 1.0 + 1e-9                           # RationalQuadratic's alpha
    caught = []
    for name, rhs in (("random", Z), ("selector", Zs)):
        good = gt.piece_errors(T, name, *gt.reference_pieces(R, dK, rhs))
        G, sld, tr, H = gt.reference_pieces(R, bad, rhs)
        if "factor 2" in mutation:
            from scipy.linalg import cho_solve
            Rinv = cho_solve((np.linalg.cholesky(R), True), np.eye(n))
            tr = np.einsum("ij,ijp->p", np.tril(Rinv), dK)
        got = gt.piece_errors(T, name, G, sld, tr, H)
        for piece in ("trace", "H"):
            ratio = got[piece] / (gt.BOUND * max(good[piece], EPS))
            print(f"{mutation}: {name} {piece}: e = {got[piece] / EPS:.3g} eps = {ratio:.3g} x the bound")
            caught.append(ratio > 1.0)
    assert any(caught)
    if "scaled" in mutation or "anisotropic" in mutation:
        assert caught[3]                                     # ... and the selector's H_p alone pins it
