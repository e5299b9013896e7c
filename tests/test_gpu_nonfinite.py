"""The main library on non-finite and degenerate inputs, on every likelihood route (inputs and expectations:
tests/nonfinite_cases.py, proved on the CPU by tests/test_nonfinite_cpu.py).

* a NaN or infinite point: the built entries have scikit-learn's classes, info is netlib's first refused pivot on k_lml_small,
  k_lml_medium, the grouped schedule (zero flags, envelope and live-tile lists on and off), the single-factorisation schedules,
  k_grad_small, the general gradient path, both gradient-batch routes and gsum_potrf_lower; gradient pieces are zeros there;
* members of a batch are independent of a failing neighbour, bit for bit;
* a non-finite right-hand-side entry stays in its column (and, where the operator is causal, below its 16-row micro-block);
* the strict upper triangle of an uploaded matrix never reaches a result;
* the exactly diagonal kernel C(a) RBF(1e-3) + White(w) against its closed form in long double, inside derived bounds, on every route.

Nothing here can fault: the inputs are data, every extent, wait and launch shape is independent of the values."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from sklearn.gaussian_process.kernels import RBF, ConstantKernel as C, Matern, WhiteKernel

import gsum_amd as gm
import nonfinite_cases as nc
from conftest import record_parity
from gsum_amd.kernels import describe_gradient, describe_kernel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return gm.default_context(0)


@pytest.fixture(scope="module")
def lab():
    return gm.lab_context(0)


class options:
    """Set lab options for a block and put back what the context held before (read first: the lab context is shared by the process)."""

    def __init__(self, c, opts):
        self.c, self.opts = c, opts

    def __enter__(self):
        self.saved = {name: self.c.get_option(name) for name in self.opts}
        for name, value in self.opts.items():
            self.c.set_option(name, value)

    def __exit__(self, *exc):
        for name, value in self.saved.items():
            self.c.set_option(name, value)


def _desc(kernel):
    return describe_kernel(kernel, 1)


GROUPED = {
    "grouped_all_on": dict(wave_skip_zero=1, wave_env=1, wave_far_plan=1),
    "grouped_flags_only": dict(wave_skip_zero=1, wave_env=0, wave_far_plan=0),
    "grouped_all_off": dict(wave_skip_zero=0, wave_env=0, wave_far_plan=0),
}
SINGLE_SCHEDULES = {
    "host": dict(chain_persist=0, lookahead=1, chain_fused=1),
    "lazy": dict(chain_persist=0, lookahead=0, lazy_min_np=1024, lazy_far=2),
    "chain": dict(chain_persist=1, chain_rows=256, chain_lazy=1),
    "deep": dict(chain_persist=1, chain_deep=1, chain_deep_rows=0, chain_depth=2),
}


def value_routes(n):
    """name -> lab options that send a gsum_lml_batch call of any size down that route (host/api_lml.hip.h)"""
    if n <= 128:
        return {"small": {}}
    routes = {}
    if n in nc.MEDIUM:
        routes["medium"] = dict(medium_path=1, medium_min_batch=1)
    for name, flags in GROUPED.items():
        routes[name] = dict(medium_path=0, wave_min=1, **flags)
    routes["single"] = dict(medium_path=0, wave_min=1000)
    return routes


def grad_batch_routes(n):
    """gsum_lml_grad_batch: k_grad_small up to 128; above it the slot pipeline, and beyond 256 the grouped factorisations too"""
    if n <= 128:
        return {"grad_small": {}}
    routes = {"slots": dict(wave_min=1000)}
    if n > 256:
        routes["grouped"] = dict(wave_min=2)
    return routes


def _assert_bits(got, want):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(want).view(np.int64))


def _nonfinite(a):
    return not np.any(np.isfinite(a))


# ---- 1. the build: scikit-learn's entry classes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (17, 129, 385))
@pytest.mark.parametrize("name", list(nc.KERNELS))
def test_build_classes_of_a_nonfinite_point(ctx, name, n):
    kernel = nc.KERNELS[name]()
    desc = _desc(kernel)
    for value in nc.NONFINITE:
        for i in sorted({0, n // 2, n - 1}):
            X = nc.plant_point(nc.grid(n), i, value)
            want = nc.classes(nc.sk_matrix(kernel, X))
            np.testing.assert_array_equal(nc.classes(ctx.kernel_matrix(desc, X, diag_add=nc.NUGGET)), want)
            M = ctx.kernel_matrix_dev(desc, X, diag_add=nc.NUGGET)
            try:
                low = np.tril_indices(n)
                np.testing.assert_array_equal(nc.classes(M.to_host())[low], want[low])
            finally:
                M.free()
            Xs = nc.plant_point(0.05 + nc.grid(37), 11, value)                       # the two-argument form: column 11 only
            with np.errstate(all="ignore"):
                cross = kernel(nc.grid(n), Xs)
            np.testing.assert_array_equal(nc.classes(ctx.kernel_matrix(desc, nc.grid(n), Xs)), nc.classes(cross))


@pytest.mark.parametrize("n", (129, 385, 641))
def test_infinite_point_under_a_banded_matern_is_nan_or_zero(ctx, lab, n):
    """The one place where the build's classes differ from scikit-learn's (section 25).  Matern(0.01) on the 0.1 grid underflows from
    lag 44 on, and a wave of k_build2 whose 2 x 128 entries all have an exponential of exactly zero stores amplitude * 0 + constant
    without evaluating the polynomial factor (gs_plain_pair's wave-uniform short cut).  For an infinite point scikit-learn's factor is
    inf and its entry inf * 0 = NaN; the short cut leaves 0.0 there.  Pinned as found: such an entry is NaN or exactly zero, every other
    entry has scikit-learn's class, row and column i keep NaN beside the diagonal (the diagonal tile takes no short cut) -- and so
    info is netlib's on every route."""
    kernel = Matern(0.01, nu=1.5)
    desc = _desc(kernel)
    for value in (np.inf, -np.inf):
        for i in sorted({0, n // 2, n - 1}):
            X = nc.plant_point(nc.grid(n), i, value)
            want = nc.classes(nc.sk_matrix(kernel, X))
            got = nc.classes(ctx.kernel_matrix(desc, X, diag_add=nc.NUGGET))
            differ = got != want
            assert np.all(want[differ] == 4) and np.all(got[differ] == 0)
            rows, cols = np.nonzero(differ)
            assert np.all((rows == i) | (cols == i))
            near = [j for j in (i - 1, i + 1) if 0 <= j < n]
            assert np.all(got[i, near] == 4) and np.all(got[near, i] == 4)
            for route, opts in value_routes(n).items():
                with options(lab, opts):
                    assert lab.lml_batch([desc] * 3, X, nc.rhs(n), nc.NUGGET)[2].tolist() == [nc.info_of_nan_point(n, i)] * 3, route


@pytest.mark.parametrize("n", (17, 129, 385))
def test_build_of_degenerate_hyperparameters(ctx, n):
    """length scale 1e300 or inf: all ones; amplitude 0: zeros; C(a) RBF(1e-3) + White(w): s I with s in the build's association"""
    X = nc.grid(n)
    for name, (kernel, _) in nc.bad_members().items():
        _assert_bits(ctx.kernel_matrix(_desc(kernel), X) + 0.0, nc.sk_matrix(kernel, X, 0.0) + 0.0)
    for a in (nc.CLOSED_A, 0.0):
        kernel = nc.closed_kernel(a)
        want = nc.closed_scale(a) * np.eye(n)
        _assert_bits(ctx.kernel_matrix(_desc(kernel), X, diag_add=nc.NUGGET) + 0.0, want)
        M = ctx.kernel_matrix_dev(_desc(kernel), X, diag_add=nc.NUGGET)
        try:
            _assert_bits(np.tril(M.to_host()) + 0.0, want)
        finally:
            M.free()


def test_refused_length_scales(ctx):
    """describe_kernel refuses them for every backend (tests/test_nonfinite_cpu.py); a descriptor made by hand meets the library's own
    refusal, the same ValueError"""
    for ls in nc.REFUSED_LENGTH_SCALES:
        kernel = RBF(1.0)
        kernel.length_scale = ls
        with pytest.raises(ValueError, match="length_scale"):
            describe_kernel(kernel, 1)
        desc = _desc(RBF(1.0))
        desc.length_scale[0] = ls
        with pytest.raises(ValueError, match="length_scale"):
            ctx.lml_batch([desc], nc.grid(17), nc.rhs(17), nc.NUGGET)


# ---- 2. info of a non-finite point on every value route ---------------------------------------------------------------------------------
def _trio():
    return [_desc(nc.KERNELS[name]()) for name in ("banded", "dense", "tree")]


@pytest.mark.parametrize("n", nc.ONE_WORKGROUP + nc.MEDIUM + nc.LARGE)
def test_nan_point_info_on_every_value_route(lab, n):
    descs, Z = _trio(), nc.rhs(n)
    for route, opts in value_routes(n).items():
        with options(lab, opts):
            assert not np.any(lab.lml_batch(descs, nc.grid(n), Z, nc.NUGGET)[2]), route
            for i in nc.plant_rows(n):
                info = lab.lml_batch(descs, nc.plant_point(nc.grid(n), i), Z, nc.NUGGET)[2]
                assert list(info) == [nc.info_of_nan_point(n, i)] * 3, (route, i)


@pytest.mark.parametrize("n", (2, 17, 129, 385, 641))
def test_infinite_point_info_on_every_value_route(lab, n):
    """RBF: row i is exactly zero, a valid matrix (info 0, finite results); Matern-3/2: inf * 0 = NaN, the NaN point's info"""
    descs, Z = [_desc(nc.banded()), _desc(nc.dense())], nc.rhs(n)
    for route, opts in value_routes(n).items():
        with options(lab, opts):
            for value in (np.inf, -np.inf):
                for i in sorted({0, n // 2, n - 1}):
                    G, sld, info = lab.lml_batch(descs, nc.plant_point(nc.grid(n), i, value), Z, nc.NUGGET)
                    assert list(info) == [0, nc.info_of_nan_point(n, i)], (route, value, i)
                    assert np.all(np.isfinite(G[0])) and np.isfinite(sld[0])


@pytest.mark.parametrize("n", (2, 17, 128, 129, 257, 385, 641, 1100))
def test_all_ones_and_zero_members_info(lab, n):
    """nugget 0: the all-ones matrix stops at pivot 1 (1 - 1 = 0 exactly), the zero matrix at pivot 0, on every route"""
    members = nc.bad_members()
    descs = [_desc(k) for k, _ in members.values()]
    want = [w for _, w in members.values()]
    for route, opts in value_routes(n).items():
        with options(lab, opts):
            assert list(lab.lml_batch(descs, nc.grid(n), nc.rhs(n), 0.0)[2]) == want, route


@functools.lru_cache(maxsize=None)
def _planted_matrix(name, n, i):
    """scikit-learn's matrix with X[i] = NaN (computed once: shared by the potrf tests, never written to)"""
    K = nc.sk_matrix(nc.KERNELS[name](), nc.plant_point(nc.grid(n), i))
    K.setflags(write=False)
    return K


def _potrf_info(c, A):
    M = c.upload(A)
    try:
        return c.potrf(M)
    finally:
        M.free()


@pytest.mark.parametrize("n", nc.ONE_WORKGROUP + nc.MEDIUM + nc.LARGE)
def test_nan_point_info_potrf(ctx, n):
    """gsum_potrf_lower on scikit-learn's own matrix (uploaded) and on the device's build (factorize), product context"""
    for name in (("dense",) if n in nc.LARGE else ("banded", "dense")):
        kernel = nc.KERNELS[name]()
        for i in nc.plant_rows(n):
            X = nc.plant_point(nc.grid(n), i)
            want = nc.info_of_nan_point(n, i)
            assert _potrf_info(ctx, _planted_matrix(name, n, i)) == want, (name, i)
            M, info = ctx.factorize(_desc(kernel), X, diag_add=nc.NUGGET)
            M.free()
            assert info == want, (name, i)


@pytest.mark.parametrize("family", list(SINGLE_SCHEDULES))
@pytest.mark.parametrize("n", nc.LARGE)
def test_nan_point_info_single_schedules(lab, n, family):
    with options(lab, SINGLE_SCHEDULES[family]):
        for i in nc.plant_rows(n):
            assert _potrf_info(lab, _planted_matrix("dense", n, i)) == nc.info_of_nan_point(n, i), i


# ---- 3. the gradient routes: info, and zeros where info > 0 -----------------------------------------------------------------------------
def _grad_kernels():
    return [C(1.0) * RBF(0.2) + WhiteKernel(1e-6), C(1.5) * Matern(5.0, nu=1.5) + WhiteKernel(1e-6), C(0.7) * RBF(0.35) + WhiteKernel(1e-6)]


@pytest.mark.parametrize("n", nc.GRADIENT)
def test_nan_point_gradient_routes(lab, n):
    kernels = _grad_kernels()
    descs, params = [_desc(k) for k in kernels], [describe_gradient(k, 1) for k in kernels]
    Z = nc.rhs(n)
    for i in nc.plant_rows(n):
        X = nc.plant_point(nc.grid(n), i)
        want = nc.info_of_nan_point(n, i)
        for d, p in zip(descs[:2], params[:2]):                                    # k_grad_small / the general path
            G, sld, info, trace, H = lab.lml_grad(d, p, X, Z, 0.0)
            assert info == want, i
            assert not np.any(trace) and not np.any(H)
        for route, opts in grad_batch_routes(n).items():
            with options(lab, opts):
                G, sld, info, trace, H = lab.lml_grad_batch(descs, params, X, Z, 0.0)
                assert list(info) == [want] * 3, (route, i)
                assert not np.any(trace) and not np.any(H), (route, i)


# ---- 4. members of a batch are independent ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups,size", nc.WAVE_SHAPES)
@pytest.mark.parametrize("m", nc.BATCHES)
@pytest.mark.parametrize("n,route", [(17, "small"), (129, "medium"), (257, "grouped_all_on"), (257, "grouped_all_off")])
def test_batch_members_are_independent(lab, n, route, m, groups, size):
    X, Z = nc.grid(n), nc.rhs(n)
    good = [_desc(nc.healthy(ls)) for ls in nc.batch_length_scales(m)]
    with options(lab, dict(value_routes(n)[route], wave_groups=groups, wave_size=size)):
        want = lab.lml_batch(good, X, Z, 0.0)
        assert not np.any(want[2])
        for name, (kernel, info_bad) in nc.bad_members().items():
            for pos in nc.bad_positions(m):
                descs = list(good)
                descs[pos] = _desc(kernel)
                G, sld, info = lab.lml_batch(descs, X, Z, 0.0)
                keep = np.arange(m) != pos
                assert info[pos] == info_bad, (name, pos)
                np.testing.assert_array_equal(info[keep], want[2][keep])
                _assert_bits(sld[keep], want[1][keep])
                _assert_bits(G[keep], want[0][keep])


@pytest.mark.parametrize("groups,size", nc.WAVE_SHAPES)
@pytest.mark.parametrize("m", nc.BATCHES)
@pytest.mark.parametrize("n,route", [(17, "grad_small"), (257, "slots"), (257, "grouped")])
def test_gradient_batch_members_are_independent(lab, n, route, m, groups, size):
    """trace and H too; with 23 members on 3 x 2 or 2 x 3 the grouped route takes four chunks and the slot pipeline uses every slot
    several times: the failed member sits in an earlier, the same and a later round than its neighbours"""
    X, Z = nc.grid(n), nc.rhs(n)
    good = [nc.healthy(ls) for ls in nc.batch_length_scales(m)]
    with options(lab, dict(grad_batch_routes(n)[route], wave_groups=groups, wave_size=size)):
        want = lab.lml_grad_batch([_desc(k) for k in good], [describe_gradient(k, 1) for k in good], X, Z, 0.0)
        assert not np.any(want[2])
        for name in nc.GRAD_BAD:
            kernel, info_bad = nc.bad_members()[name]
            for pos in nc.bad_positions(m):
                kernels = list(good)
                kernels[pos] = kernel
                got = lab.lml_grad_batch([_desc(k) for k in kernels], [describe_gradient(k, 1) for k in kernels], X, Z, 0.0)
                keep = np.arange(m) != pos
                assert got[2][pos] == info_bad and not np.any(got[3][pos]) and not np.any(got[4][pos]), (name, pos)
                np.testing.assert_array_equal(got[2][keep], want[2][keep])
                for a, b in zip((got[0], got[1], got[3], got[4]), (want[0], want[1], want[3], want[4])):
                    _assert_bits(a[keep], b[keep])


# ---- 5. non-finite right-hand sides ------------------------------------------------------------------------------------------------------
def _check_planted_square(got, clean, c, what):
    keep = np.arange(clean.shape[-1]) != c
    _assert_bits(got[..., keep, :][..., :, keep], clean[..., keep, :][..., :, keep])
    assert _nonfinite(got[..., c, :]) and _nonfinite(got[..., :, c]), what


@pytest.mark.parametrize("n", nc.GRADIENT)
@pytest.mark.parametrize("name", ("banded", "dense"))
def test_nonfinite_rhs_gradient(lab, name, n):
    """gsum_lml_grad (k_grad_small up to 128, the general path above): info, sld and every trace keep their bits, and so does every
    G[a, b] and H_p[a, b] away from the planted column; row and column c are non-finite throughout (NaN against inf is not promised)"""
    kernel = C(1.0) * nc.KERNELS[name]() + WhiteKernel(1e-6)
    desc, params = _desc(kernel), describe_gradient(kernel, 1)
    X, Z = nc.grid(n), nc.rhs(n)
    G0, sld0, info0, tr0, H0 = lab.lml_grad(desc, params, X, Z, 0.0)
    assert info0 == 0
    for value in nc.NONFINITE:
        for r in sorted({0, n // 2, n - 1}):
            for c in (0, Z.shape[1] - 1):
                G, sld, info, tr, H = lab.lml_grad(desc, params, X, nc.plant_rhs(Z, r, c, value), 0.0)
                assert info == 0
                _assert_bits(np.array([sld]), np.array([sld0]))
                _assert_bits(tr, tr0)
                _check_planted_square(G, G0, c, (value, r, c))
                _check_planted_square(H, H0, c, (value, r, c))
    for route, opts in grad_batch_routes(n).items():                               # gsum_lml_grad_batch: every member, every route
        with options(lab, opts):
            G0, sld0, info0, tr0, H0 = lab.lml_grad_batch([desc] * 3, [params] * 3, X, Z, 0.0)
            assert not np.any(info0), route
            for value in nc.NONFINITE:
                for r in sorted({0, n // 2, n - 1}):
                    for c in (0, Z.shape[1] - 1):
                        G, sld, info, tr, H = lab.lml_grad_batch([desc] * 3, [params] * 3, X, nc.plant_rhs(Z, r, c, value), 0.0)
                        assert not np.any(info), route
                        _assert_bits(sld, sld0)
                        _assert_bits(tr, tr0)
                        _check_planted_square(G, G0, c, (route, value, r, c))
                        _check_planted_square(H, H0, c, (route, value, r, c))


@pytest.mark.parametrize("n", nc.GRADIENT)
def test_all_ones_member_info_gradient_routes(lab, n):
    """length scale 1e300 or inf, no noise to speak of, nugget 0: info == 2 and zero pieces on k_grad_small, the general path and
    every route of the gradient batch"""
    kernels = [nc.bad_members()[name][0] for name in nc.GRAD_BAD] + [nc.bad_members()[nc.GRAD_BAD[0]][0]]
    descs, params = [_desc(k) for k in kernels], [describe_gradient(k, 1) for k in kernels]
    X, Z = nc.grid(n), nc.rhs(n)
    for d, p in zip(descs[:2], params[:2]):
        G, sld, info, trace, H = lab.lml_grad(d, p, X, Z, 0.0)
        assert info == 2 and not np.any(trace) and not np.any(H)
    for route, opts in grad_batch_routes(n).items():
        with options(lab, opts):
            G, sld, info, trace, H = lab.lml_grad_batch(descs, params, X, Z, 0.0)
            assert list(info) == [2, 2, 2] and not np.any(trace) and not np.any(H), route


@pytest.mark.parametrize("n", (17, 128, 129, 257, 641))
@pytest.mark.parametrize("name", ("banded", "dense"))
def test_nonfinite_rhs_value_routes(lab, name, n):
    descs = [_desc(nc.KERNELS[name]())] * 3
    X, Z = nc.grid(n), nc.rhs(n)
    for route, opts in value_routes(n).items():
        with options(lab, opts):
            G0, sld0, info0 = lab.lml_batch(descs, X, Z, nc.NUGGET)
            assert not np.any(info0)
            for value in nc.NONFINITE:
                for r in sorted({0, n // 2, n - 1}):
                    for c in (0, Z.shape[1] - 1):
                        G, sld, info = lab.lml_batch(descs, X, nc.plant_rhs(Z, r, c, value), nc.NUGGET)
                        assert not np.any(info), route
                        _assert_bits(sld, sld0)
                        _check_planted_square(G, G0, c, (route, value, r, c))


@pytest.mark.parametrize("k", (1, 4))
@pytest.mark.parametrize("n", (17, 129, 257, 641))
def test_rhs_whose_only_nonzero_is_nonfinite(lab, n, k):
    """Right-hand sides of zeros but for one NaN or infinite entry: the border group's only entry that is not +-0 is not finite.  It
    counts as nonzero (gs_panel16_any's rule), so the group is solved and its corner tile runs: row and column c of G are non-finite
    on every route, the rest of G is zero."""
    descs = [_desc(nc.banded()), _desc(nc.dense())]
    X = nc.grid(n)
    for route, opts in value_routes(n).items():
        with options(lab, opts):
            for value in nc.NONFINITE:
                for r in sorted({0, n // 2, n - 1}):
                    c = k - 1
                    G, sld, info = lab.lml_batch(descs, X, nc.plant_rhs(np.zeros((n, k)), r, c, value), nc.NUGGET)
                    assert not np.any(info), route
                    keep = np.arange(k) != c
                    assert _nonfinite(G[:, c, :]) and _nonfinite(G[:, :, c]), (route, value, r)
                    assert not np.any(G[:, keep][:, :, keep]), (route, value, r)


# ---- 6. operators on a factor ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operator_inputs(n, k):
    rng = np.random.RandomState(100 + k)
    return dict(X=nc.grid(n), Z=rng.randn(n, k), mean=rng.randn(n), Xs=0.05 + nc.grid(37) * (n / 37.0))


def _micro(r):
    return 16 * (r // 16)


@pytest.mark.parametrize("k", nc.OPERATOR_K)
@pytest.mark.parametrize("n", nc.OPERATOR)
def test_operators_keep_a_nonfinite_entry_in_its_column(ctx, n, k):
    """forward_solve, sqrt_errors and tri_multiply are causal: above the planted row column c keeps its bits -- for tri_multiply
    from row r, for the two solves from the planted row's 16-row micro-block 16 (r // 16) (the panel kernel multiplies a micro-block by
    the stored inverse of its diagonal block, zeros of its upper triangle included: 0 * NaN; section 25)."""
    I = _operator_inputs(n, k)
    desc = _desc(nc.dense())
    L, info = ctx.factorize(desc, I["X"], diag_add=nc.NUGGET)
    assert info == 0
    try:
        def run(Z):
            out = dict(W=ctx.forward_solve(L, Z), G=ctx.forward_gram(L, Z)[0], LZ=ctx.tri_multiply(L, Z))
            out["E"], out["md2"] = ctx.sqrt_errors(L, Z, I["mean"], pivot=False, md2=True)
            out["css"], out["VtW"], _ = ctx.predict_terms(L, desc, I["X"], I["Xs"], rhs=Z)
            out["css2"], vtw = ctx.predict_var(L, desc, I["X"], I["Xs"], want_vtw=True)
            out["VtW2"] = vtw[:, :k]
            out["S"] = ctx.cho_solve(L, Z)
            return out

        clean = run(I["Z"])
        for value in nc.NONFINITE:
            for r in sorted({0, 77, n - 1}):
                for c in sorted({0, k - 1}):
                    got = run(nc.plant_rhs(I["Z"], r, c, value))
                    keep = np.arange(k) != c
                    what = (value, r, c)
                    for key in ("W", "LZ", "E", "VtW", "VtW2", "S"):
                        _assert_bits(got[key][:, keep], clean[key][:, keep])
                    _assert_bits(got["md2"][keep], clean["md2"][keep])
                    _assert_bits(got["css"], clean["css"])
                    _assert_bits(got["css2"], clean["css2"])
                    _check_planted_square(got["G"], clean["G"], c, what)
                    _assert_bits(got["LZ"][:r, c], clean["LZ"][:r, c])
                    for key in ("W", "E"):
                        _assert_bits(got[key][:_micro(r), c], clean[key][:_micro(r), c])
                        assert _nonfinite(got[key][r:, c]), (key, what)
                    assert _nonfinite(got["LZ"][r:, c]) and _nonfinite(got["S"][:, c]), what
                    assert _nonfinite(got["VtW"][:, c]) and _nonfinite(got["VtW2"][:, c]) and not np.isfinite(got["md2"][c]), what
    finally:
        L.free()


@pytest.mark.parametrize("n", nc.OPERATOR)
def test_a_nonfinite_new_point_stays_in_its_row(ctx, n):
    I = _operator_inputs(n, 5)
    desc = _desc(nc.dense())
    L, info = ctx.factorize(desc, I["X"], diag_add=nc.NUGGET)
    assert info == 0
    try:
        def run(Xs):
            css, VtW, cov = ctx.predict_terms(L, desc, I["X"], Xs, rhs=I["Z"], want_cov=True)
            css2, vtw2 = ctx.predict_var(L, desc, I["X"], Xs, want_vtw=True)
            return css, VtW, cov, css2, vtw2[:, :5]

        clean = run(I["Xs"])
        m = I["Xs"].shape[0]
        for value in nc.NONFINITE:
            for q in (0, 16, m - 1):
                got = run(nc.plant_point(I["Xs"], q, value))
                keep = np.arange(m) != q
                for j in (0, 1, 3, 4):
                    _assert_bits(got[j][keep], clean[j][keep])
                _assert_bits(got[2][keep][:, keep], clean[2][keep][:, keep])
                # Matern-3/2: a NaN or infinite new point gives a NaN column of kernel(X, Xs) (inf * 0)
                assert np.isnan(got[0][q]) and np.isnan(got[3][q]) and _nonfinite(got[1][q]) and _nonfinite(got[4][q])
                assert _nonfinite(got[2][q]) and _nonfinite(got[2][:, q])
    finally:
        L.free()


# ---- 7. uplo = 'L' -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (129, 257))
def test_upper_triangle_never_reaches_a_result(ctx, n):
    A = nc.sk_matrix(nc.dense(), nc.grid(n))
    Z = nc.rhs(n)

    def run(B):
        M = ctx.upload(B)
        try:
            info = ctx.potrf(M)
            return info, M.to_host(), ctx.forward_gram(M, Z)
        finally:
            M.free()

    info0, L0, (G0, sld0) = run(A)
    assert info0 == 0 and not np.any(np.triu(L0, 1))
    for r, c in nc.upper_plants(n):
        B = A.copy()
        B[r, c] = np.nan
        info, L, (G, sld) = run(B)
        assert info == 0, (r, c)
        _assert_bits(L, L0)
        _assert_bits(G, G0)
        assert sld == sld0


# ---- 8. the exactly diagonal kernel against its closed form -----------------------------------------------------------------------------
def _check_closed(name, cf, G, sld, trace=None, H=None, order=None):
    ratios = nc.closed_ratios(cf, G, sld, trace, H, order)
    record_parity(name, **ratios)
    assert all(r <= 1.0 for r in ratios.values()), (name, ratios)              # (every ratio by itself: a NaN fails the comparison)
    if order is not None:
        p = order.index("length")
        assert trace[p] == 0.0 and not np.any(H[p]), name


@pytest.mark.parametrize("a", (nc.CLOSED_A, 0.0))
@pytest.mark.parametrize("n", nc.ONE_WORKGROUP + nc.MEDIUM + nc.LARGE)
def test_closed_form_value_routes(lab, n, a):
    desc = _desc(nc.closed_kernel(a))
    X, Z = nc.grid(n), nc.rhs(n)
    cf = nc.closed_form(Z, a)
    M = lab.kernel_matrix_dev(desc, X, diag_add=nc.NUGGET)
    try:
        _assert_bits(np.tril(M.to_host()) + 0.0, cf["s"] * np.eye(n))               # the association of closed_scale is the build's
    finally:
        M.free()
    for route, opts in value_routes(n).items():
        with options(lab, opts):
            G, sld, info = lab.lml_batch([desc] * 3, X, Z, nc.NUGGET)
            assert not np.any(info), route
            for j in (1, 2):
                _assert_bits(G[j], G[0])
            _check_closed(f"closed_form_a{a:g}_n{n}_{route}", cf, G[0], sld[0])
    if n in nc.LARGE:                    # the single-factorisation schedules: the fused evaluation, and potrf + forward_gram on the built matrix
        for family, sched in SINGLE_SCHEDULES.items():
            with options(lab, dict(value_routes(n)["single"], **sched)):
                G, sld, info = lab.lml_batch([desc], X, Z, nc.NUGGET)
                assert info[0] == 0, family
                _check_closed(f"closed_form_a{a:g}_n{n}_single_{family}", cf, G[0], sld[0])
                M = lab.kernel_matrix_dev(desc, X, diag_add=nc.NUGGET)
                try:
                    assert lab.potrf(M) == 0, family
                    G, sld = lab.forward_gram(M, Z)
                finally:
                    M.free()
                _check_closed(f"closed_form_a{a:g}_n{n}_potrf_{family}", cf, G, sld)


@pytest.mark.parametrize("n", nc.MEDIUM + nc.LARGE)
def test_closed_form_dead_work_counters(lab, n):
    """On the grouped schedule every panel row group of a diagonal matrix but the border's (the right-hand sides: they always run)
    is dead: each of the np / 256 panel steps of each member loads one group.  Every far tile of the MATRIX rows is dead: with
    right-hand sides of zeros no tile is listed at all.  With nonzero right-hand sides a far update keeps one live tile per member,
    the corner (border x border, C -= W_p W_p^T: the tile G is accumulated in) -- the only one with a flagged group on both sides."""
    desc = _desc(nc.closed_kernel())
    X = nc.grid(n)
    S = -(-n // 256)
    for Z in (nc.rhs(n), np.zeros((n, 4))):
        with options(lab, dict(value_routes(n)["grouped_all_on"], profile_gemm=1)):
            lab.kernel_profile()
            info = lab.lml_batch([desc] * 3, X, Z, nc.NUGGET)[2]
            prof = lab.kernel_profile()
        assert not np.any(info)
        panel, bulk = prof["panel_gemm"], prof["bulk_update"]
        record_parity(f"closed_form_counters_n{n}_{'rhs' if np.any(Z) else 'zero_rhs'}", panel_groups=panel["panel_groups"],
                      panel_groups_loaded=panel["panel_groups_loaded"], tiles=bulk["tiles"], tiles_run=bulk["tiles_run"],
                      tiles_listed=bulk["tiles_listed"])
        assert panel["panel_groups"] == 3 * sum((256 * S + 16 - 256 * (s + 1)) // 16 for s in range(S))
        assert panel["panel_groups_loaded"] == 3 * S
        assert bulk["tiles_listed"] == bulk["tiles_run"]
        if np.any(Z):
            assert 0 < bulk["tiles_listed"] <= 3 * S                     # (at most one far update per member and panel step)
        else:
            assert bulk["tiles_listed"] == 0


@pytest.mark.parametrize("a", (nc.CLOSED_A, 0.0))
@pytest.mark.parametrize("n", nc.GRADIENT)
def test_closed_form_gradient_routes(lab, n, a):
    kernel = nc.closed_kernel(a)
    order = nc.gradient_order(kernel)
    desc, params = _desc(kernel), describe_gradient(kernel, 1)
    X, Z = nc.grid(n), nc.rhs(n)
    cf = nc.closed_form(Z, a)
    G, sld, info, trace, H = lab.lml_grad(desc, params, X, Z, nc.NUGGET)
    assert info == 0
    _check_closed(f"closed_form_a{a:g}_n{n}_lml_grad", cf, G, sld, trace, H, order)
    for route, opts in grad_batch_routes(n).items():
        with options(lab, opts):
            G, sld, info, trace, H = lab.lml_grad_batch([desc] * 3, [params] * 3, X, Z, nc.NUGGET)
            assert not np.any(info), route
            _check_closed(f"closed_form_a{a:g}_n{n}_grad_batch_{route}", cf, G[1], sld[1], trace[1], H[1], order)
