"""The exact-factor designs (tests/exact_factors.py) and the checks built on them, proven without a GPU: the designs meet their
exactness conditions, the closed forms equal rational arithmetic, and ``backend='cpu'`` (LAPACK / scipy, exact on these inputs) passes
the very helper functions the device tests run -- operators, info codes, call sequences and the state contract of the operator level."""
import numpy as np
import pytest
from scipy.linalg import cho_solve, solve_triangular

import exact_factors as xf
from gsum_amd import describe_kernel
from gsum_amd._cpu import CpuContext
from sklearn.gaussian_process.kernels import RBF


@pytest.fixture(scope="module")
def ctx():
    return CpuContext()


@pytest.fixture(scope="module")
def desc():
    return describe_kernel(RBF(0.3), 1)


@pytest.mark.parametrize("n,part", xf.OPERATOR_CASES)
def test_designs_meet_their_exactness_conditions(n, part):
    """Every design of the device's section 1 (and, through the helpers below, of the others): the conditions hold with room, the
    structure is as described, and LAPACK / scipy reproduce the closed forms bit for bit."""
    d = xf.design(n, part)
    Z, B, Y, mean = xf.operator_inputs(d)
    assert max(d.bits.values()) <= 53
    assert set(np.unique(d.N)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert d.e.min() >= -2 and d.e.max() <= 5
    xf.eq(np.diag(d.L) ** 2, 4.0 ** d.e)                          # every pivot is 4^e
    xf.eq(d.A * 16.0, np.rint(d.A * 16.0))                        # multiples of 2^-4
    Lr = np.linalg.cholesky(d.A)
    xf.eq(Lr, d.L)
    xf.eq(solve_triangular(Lr, Z, lower=True), d.W(Z))
    xf.eq(cho_solve((Lr, True), B), d.X(B))
    W = d.W(Z)
    xf.eq(W.T @ W, d.G(Z))
    xf.eq(d.L.T @ d.X(B), d.W(B))                                 # X = L^-T W, by multiplication
    d.check_sld(np.log(np.diag(Lr)).sum())


def test_partitions_are_what_they_say():
    d = xf.design(64, "alt")
    assert d.N[1::2, 0::2].any() and not d.N[0::2, :].any() and not d.N[:, 1::2].any()
    assert np.count_nonzero(np.tril(d.N[:16, :16], -1))           # sub-diagonal content inside a diagonal micro-block
    d = xf.design(64, "blocks16")
    for b in range(4):
        assert not d.N[16 * b:16 * b + 16, 16 * b:16 * b + 16].any()          # diagonal micro-blocks are diagonal
    assert d.N[16:32, 0:16].any() and d.N[48:64, 32:48].any()
    d = xf.design(64, "rand")
    assert not d.N[0].any()
    for dd in (xf.design(64, p) for p in xf.PARTITIONS):
        assert not dd.N[dd.s1].any() and not dd.N[:, ~dd.s1].any()             # sinks take from sources only: N^2 = 0
        for i in np.nonzero(~dd.s1)[0]:
            assert dd.N[i].any() == bool(dd.s1[:i].any())                         # at least one nonzero where there is a source to the left


@pytest.mark.parametrize("n,part", [c for c in xf.OPERATOR_CASES if c[0] <= 129])
def test_closed_forms_equal_fraction_arithmetic(n, part):
    d = xf.design(n, part)
    Z = xf.operands(n, 3, 1)
    Lf, Wf, Xf, Gf = xf.fraction_reference(d.A, Z)
    xf.eq(d.L, Lf)
    xf.eq(d.W(Z), Wf)
    xf.eq(d.X(Z), Xf)
    xf.eq(d.G(Z), Gf)


@pytest.mark.parametrize("n,k", xf.SWEEP_CASES)
def test_sweep_designs_are_exact(n, k):
    d = xf.design(n, "rand", 3)
    Y = xf.operands(n, k, 9)
    mean = xf.operands(n, 1, 10)[:, 0]
    d.check(Y=Y, mean=mean)
    E = solve_triangular(d.L, Y - mean[:, None], lower=True)
    xf.eq(E, d.W(Y - mean[:, None]))


@pytest.mark.parametrize("refused", [True, False])
@pytest.mark.parametrize("n", [385, 1025])
def test_guard_designs_are_exact(n, refused):
    g, j = xf.guard_design(n, refused)
    assert g.bits["|L||L|^T"] <= 53
    xf.eq(np.linalg.cholesky(g.A), g.L)                           # (LAPACK has no guard: both factorise)
    assert 2.0 ** -51 * g.A[j, j] == (1.0 + 2.0 ** -51 if refused else 0.5 + 2.0 ** -51)


@pytest.mark.parametrize("n,part", xf.OPERATOR_CASES)
def test_operators_cpu_backend(ctx, n, part):
    xf.check_operators(ctx, xf.design(n, part))


@pytest.mark.parametrize("n", xf.INFO_ORDERS)
def test_info_cpu_backend(ctx, n):
    d = xf.design(n, "rand", 4)
    for cols, twice in xf.info_cases(n):
        xf.check_info(ctx, d, cols, twice)


@pytest.mark.parametrize("n", xf.SEQUENCE_ORDERS)
def test_call_sequences_cpu_backend(ctx, n):
    xf.check_sequences(ctx, n)


def test_refusals_cpu_backend(ctx, desc):
    xf.check_refusals(ctx, desc)


def test_predict_var_contract_cpu_backend(ctx, desc):
    xf.check_predict_var_contract(ctx, desc)


def test_blocked_algorithm_is_exact_on_a_design():
    """The numpy emulation of the device's bordered right-looking algorithm (tests/test_blocked_algorithm.py): array_equal, not
    allclose -- the algebra itself, with explicit block inverses, border rows and the corner, loses nothing on an exact design."""
    from test_blocked_algorithm import emulate
    for n, part in ((200, "alt"), (391, "rand"), (385, "blocks16")):
        d = xf.design(n, part, 2)
        Z = xf.operands(n, 5, 5)
        d.check(Z=Z)
        L, W, G, sld = emulate(d.A, Z)
        xf.eq(L, d.L)
        xf.eq(W, d.W(Z))
        xf.eq(G, d.G(Z))
        d.check_sld(sld)
