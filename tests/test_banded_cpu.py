"""The banded likelihood path without a device: backend='cpu' through the exact factors, the derived bounds and the model value of
banded_cases.py, the contract of libgsum_band.so on a null or fake handle, the Python layer's checks and the model layer's refusals.
DESIGN.md section 26."""
import ctypes as C_
import os
import re

import numpy as np
import pytest
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, DotProduct, ExpSineSquared, Matern, RationalQuadratic

import banded_cases as bc
import gsum_amd as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_CPU, W_CPU = 16, 255                                                # the device library's constants: the cpu backend has no edges of its own


def test_the_library_is_the_sixth_side_library_and_exports_its_header():
    from gsum_amd import _band_lib, build
    assert "band" in build.SIDE and list(build.SIDE)[5] == "band" and len(build.SIDE) == 6
    header = open(os.path.join(ROOT, "include", "gsum_band.h")).read()
    declared = set(re.findall(r"\b(gsum_band_\w+)\s*\(", header.split("#ifndef GSUM_BAND_H")[1]))
    assert declared == set(_band_lib.PROTOTYPES)
    lib = _band_lib.load_library()
    for name in declared:
        assert hasattr(lib, name)
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _band_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()}
    assert {s for s in exported if not s.startswith("_")} == declared and all(s.startswith("gsum_band_") for s in exported)
    deps = build.SIDE_EXTRA["band"]
    assert any(d.endswith(os.path.join("kernels", "build.hip.h")) for d in deps) and any(d.endswith("gsum_hip.h") for d in deps)


def test_library_refuses_bad_arguments_before_it_touches_a_device():
    from gsum_amd import _band_lib
    from gsum_amd._sidelib import _d, _i32
    lib = _band_lib.load_library()
    err = lambda: lib.gsum_band_last_error().decode()  # noqa: E731
    W, B = lib.gsum_band_max_halfwidth(None), lib.gsum_band_block(None)
    assert W >= 255 and B >= 1 and W == gm.banded_max_halfwidth() and gm.banded_max_halfwidth("cpu") is None
    assert lib.gsum_band_gram(None, None, 1, 1, 0, None, 1, 1, None, None, None, None) != 0 and "null pointer" in err()
    assert lib.gsum_band_forward(None, None, 1, 1, 0, None, 1, None) != 0 and "null pointer" in err()
    assert lib.gsum_band_width(None, None, 1, None, 1, 0.0, None) != 0 and "null pointer" in err()
    assert lib.gsum_band_build(None, None, 1, None, 1, 0.0, 0, None) != 0 and "null pointer" in err()
    assert lib.gsum_band_times(None, None, 0) != 0 and "null pointer" in err()
    assert lib.gsum_band_set_chunk(None, 0) != 0 and "null pointer" in err()
    assert lib.gsum_band_open(0, None) != 0 and "null pointer" in err()
    fake = C_.c_void_p(1)                                               # never dereferenced: every refusal comes first
    n = 8
    AB, Z, out, info = np.ones((2, n)), np.ones((n, 17), order="F"), np.zeros(512), np.zeros(1, dtype=np.int32)
    ptr = lambda a: None if a is None else (_i32(a) if a.dtype == np.int32 else _d(a))  # noqa: E731

    def gram(AB_=AB, m=1, n_=n, b=1, Z_=Z, n_sets=1, cols=2, G=out, sld=out, info_=info):
        return lib.gsum_band_gram(fake, ptr(AB_), m, n_, b, ptr(Z_), n_sets, cols, ptr(G), ptr(sld), ptr(info_), None)

    for missing in (dict(Z_=None), dict(G=None), dict(sld=None), dict(info_=None)):
        assert gram(**missing) != 0 and "null pointer" in err(), missing
    for zero, word in ((dict(m=0), "m and n"), (dict(n_=0), "m and n"), (dict(n_sets=0), "n_sets")):
        assert gram(**zero) != 0 and word in err() and ">= 1" in err(), zero
    for b in (-1, W + 1):
        assert gram(b=b) != 0 and "b must be between 0 and" in err()
    for cols in (0, 17):
        assert gram(cols=cols) != 0 and "cols must be between 1 and 16" in err()
    assert gram(n_=2 ** 31 // 2, b=1) != 0 and "n * (b + 1)" in err()
    assert gram(n_=2 ** 31 // 16, b=0, cols=16) != 0 and "n * cols" in err()

    def forward(L=AB, m=1, n_=n, b=1, Z_=Z, ncols=2, Y=out):
        return lib.gsum_band_forward(fake, ptr(L), m, n_, b, ptr(Z_), ncols, ptr(Y))

    for missing in (dict(L=None), dict(Z_=None), dict(Y=None)):
        assert forward(**missing) != 0 and "null pointer" in err()
    assert forward(ncols=0) != 0 and "ncols" in err()
    assert forward(b=W + 1) != 0 and "b must be between" in err()
    assert forward(n_=2 ** 20, b=0, ncols=2 ** 11) != 0 and "n * ncols" in err()
    # descriptors: more than one feature
    from gsum_amd import describe_kernel
    two = _band_lib.desc_array([describe_kernel(RBF([0.2, 0.3]), 2)])
    one = _band_lib.desc_array([describe_kernel(RBF(0.2), 1)])
    X, w = np.arange(float(n)), np.zeros(1, dtype=np.int32)
    assert lib.gsum_band_width(fake, two, 1, _d(X), n, 0.0, _i32(w)) != 0 and "one feature" in err() and "descs[0]" in err()
    assert lib.gsum_band_build(fake, two, 1, _d(X), n, 0.0, 1, None) != 0 and "one feature" in err()
    assert lib.gsum_band_build(fake, one, 1, _d(X), n, 0.0, W + 1, None) != 0 and "b must be between" in err()
    assert lib.gsum_band_build(fake, one, 0, _d(X), n, 0.0, 1, None) != 0 and ">= 1" in err()
    assert lib.gsum_band_width(fake, one, 1, None, n, 0.0, _i32(w)) != 0 and "null pointer" in err()


def test_sorted_points():
    assert gm.sorted_points([0.0, 0.0, 1.0, 5.0]).shape == (4, 1)
    assert gm.sorted_points(np.zeros((3, 1))).shape == (3, 1)
    with pytest.raises(ValueError, match=r"X\[3\] is below X\[2\]"):
        gm.sorted_points([0.0, 1.0, 2.0, 1.5, 3.0])
    with pytest.raises(ValueError, match="not finite at index 2"):
        gm.sorted_points([0.0, 1.0, np.nan])
    with pytest.raises(ValueError, match="one feature"):
        gm.sorted_points(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="n >= 1"):
        gm.sorted_points(np.zeros(0))


def test_halfwidth_build_and_premise_on_the_cpu_backend():
    """The band against the dense matrix of the cpu backend: the same entries, the brute-force half-bandwidth, zeros outside, one
    run of nonzeros per row; the benchmark's half-bandwidth is 77."""
    from gsum_amd._cpu import kernel_matrix
    assert gm.banded_halfwidth(bc.bench_kernel(), bc.uniform_points(1025), backend="cpu") == 77
    for kernel in (bc.bench_kernel(), bc.tree_kernel()):
        for X in (bc.uniform_points(300), bc.clustered_points(300)):
            desc = gm.describe_kernel(kernel, 1)
            K = kernel_matrix(desc, X[:, None], X[:, None])
            b = gm.banded_halfwidth(kernel, X, backend="cpu")
            assert b == bc.brute_halfwidth(K) and 0 < b <= W_CPU
            AB = gm.banded_matrix(kernel, X, nugget=1e-6, backend="cpu")
            assert AB.shape == (b + 1, 300)
            np.testing.assert_array_equal(AB[1:], bc.to_band(K, b)[1:])
            np.testing.assert_array_equal(AB[0], np.full(300, float(desc.one_arg_diagonal()) + 1e-6))
            i, j = np.indices(K.shape)
            assert not np.any(K[np.abs(i - j) > b]) and bc.rows_contiguous(K)
    both = gm.banded_matrix([bc.bench_kernel(0.1), bc.bench_kernel(0.2)], bc.uniform_points(200), backend="cpu")
    assert both.shape == (2, 78, 200) and not both[0, 40:].any()
    np.testing.assert_array_equal(gm.banded_halfwidth([bc.bench_kernel(0.1), bc.bench_kernel(0.2)], bc.uniform_points(200), backend="cpu"), [38, 77])


def test_refused_kernels_and_widths():
    X = bc.uniform_points(400)
    for k in (ExpSineSquared(1.0, 2.0), RBF(0.2) * DotProduct(1.0), RBF(0.2) + ExpSineSquared(1.0, 2.0)):
        with pytest.raises(NotImplementedError, match="not monotone in distance"):
            gm.banded_halfwidth(k, X, backend="cpu")
        with pytest.raises(NotImplementedError, match="not monotone in distance"):
            gm.banded_matrix(k, X, backend="cpu")
    for k in (RBF(0.2) + ConstantKernel(1.0), RBF(5.0), RationalQuadratic(0.2, 1.0)):
        with pytest.raises(ValueError, match="half-bandwidth exceeds 255"):
            gm.banded_halfwidth(k, X, backend="cpu")
    assert gm.banded_halfwidth(Matern(0.02, nu=0.5), X, backend="cpu") == 149      # exp(-r / l) is nonzero up to r = 745.13 l
    lo, hi = bc.length_scale_at_width(lambda ls: RBF(ls), np.arange(W_CPU + 3.0), W_CPU, backend="cpu")
    assert gm.banded_halfwidth(RBF(lo), np.arange(W_CPU + 3.0), backend="cpu") == W_CPU
    with pytest.raises(ValueError, match="half-bandwidth exceeds"):
        gm.banded_matrix(RBF(hi), np.arange(W_CPU + 3.0), backend="cpu")


@pytest.mark.parametrize("b", bc.exact_widths(B_CPU, W_CPU))
def test_exact_factors_on_the_cpu_backend(b):
    """(a): every output bit for bit the planted one."""
    for k, n in enumerate(bc.exact_sizes(b, B_CPU)):
        cols, n_sets = ((1, 1), (5, 3), (16, 1))[k % 3]
        bc.check_exact("cpu", n, b, cols, n_sets)


def _bench_band(n, nugget=bc.BENCH_NUGGET):
    return gm.banded_matrix(bc.bench_kernel(), bc.uniform_points(n), nugget=nugget, backend="cpu")


def test_derived_bounds_on_the_cpu_backend():
    """(b): dpbtrf and the numpy substitution inside the componentwise bounds, on the benchmark's band and a non-uniform one."""
    AB = _bench_band(1025)
    r = bc.check_bounds("cpu", "bench n=1025", AB, bc.rough_curves(AB, 6), 1)
    assert r[0] > 1e-4                                                  # the bound is not vacuous: the residual is within four digits of it
    AB4 = _bench_band(1025, 1e-4)
    bc.check_bounds("cpu", "bench n=1025 nugget 1e-4", AB4, bc.rough_curves(AB4, 6), 2)
    ABc = gm.banded_matrix(bc.tree_kernel(), bc.clustered_points(700), backend="cpu")
    bc.check_bounds("cpu", "tree clustered n=700", ABc, bc.rough_curves(ABc, 4), 1)
    # a dropped term misses the first bound by orders of magnitude
    G, sld, info, L = gm.banded_gram(AB, np.ones((1025, 1)), return_factor=True, backend="cpu")
    Lbad = L.copy()
    Lbad[3, 500] = 0.0
    assert bc.bound_ratios(AB, Lbad, np.ones((1025, 1)), gm.banded_forward(L, np.ones((1025, 1)), backend="cpu"), G)[0] > 1e6


def test_failures_on_the_cpu_backend():
    bc.check_failures("cpu", B_CPU)


def test_model_value_on_the_cpu_backend():
    """(c): single, batch and grid entries equal each other; the value within 1e-10 of the long-double truth and 2e-10 of the dense route."""
    bc.check_model("cpu", 1025)


def test_a_matrix_that_does_not_factor_is_minus_infinity():
    X, y = bc.model_inputs(1025)
    gp = gm.ConjugateGaussianProcess(kernel=RBF(0.2), optimizer=None, nugget=-2.0, backend="cpu")
    thetas = [np.log([0.2]), np.log([0.1])]
    assert np.all(gp.log_marginal_likelihood_batch(thetas, X=X[:200], y=y[:200], structure="banded") == -np.inf)
    assert gp.log_marginal_likelihood(thetas[0], X=X[:200], y=y[:200], structure="banded") == -np.inf


def test_model_layer_refusals():
    X, y = bc.model_inputs(1025)
    X, y = X[:300], y[:300, :3]
    gp = bc.model_process("cpu")
    th = np.log([0.2])
    for call in (lambda s: gp.log_marginal_likelihood(th, X=X, y=y, structure=s), lambda s: gp.log_marginal_likelihood_batch([th], X=X, y=y, structure=s)):
        with pytest.raises(ValueError, match="structure"):
            call("circulant")
    with pytest.raises(NotImplementedError, match="gradient"):
        gp.log_marginal_likelihood(th, eval_gradient=True, X=X, y=y, structure="banded")
    with pytest.raises(NotImplementedError, match="gradient"):
        gp.log_marginal_likelihood_batch([th], X=X, y=y, structure="banded", eval_gradient=True)
    with pytest.raises(NotImplementedError, match="banded"):
        bc.model_process("cpu").fit(X, y, structure="banded")
    fitted = bc.model_process("cpu").fit(X, y)
    with pytest.raises(NotImplementedError, match="banded"):
        fitted.predict(X[:3], structure="banded")
    with pytest.raises(NotImplementedError, match="banded"):
        fitted.loo(structure="banded")
    with pytest.raises(ValueError, match="at most 15 curves"):
        gp.log_marginal_likelihood(th, X=X, y=np.ones((300, 16)), structure="banded")
    Xu = X.copy()
    Xu[[7, 8]] = Xu[[8, 7]]
    with pytest.raises(ValueError, match=r"X\[8\] is below X\[7\]"):
        gp.log_marginal_likelihood(th, X=Xu, y=y, structure="banded")
    with pytest.raises(ValueError, match=r"\(n, 1\)"):
        gp.log_marginal_likelihood(th, X=np.random.RandomState(0).rand(300, 2), y=y, structure="banded")
    with pytest.raises(ValueError, match="half-bandwidth exceeds"):
        gp.log_marginal_likelihood(np.log([5.0]), X=X, y=y, structure="banded")
    periodic = gm.ConjugateGaussianProcess(kernel=ExpSineSquared(1.0, 2.0), optimizer=None, backend="cpu")
    with pytest.raises(NotImplementedError, match="not monotone"):
        periodic.log_marginal_likelihood(None, X=X, y=y, structure="banded")
    tg = bc.truncation_process("cpu", X, y)
    for kw in (dict(structure="circulant"), dict(structure="banded", devices="all"), dict(structure="banded", gather="rccl"),
               dict(structure="banded", mode="fast"), dict(structure="banded", X=Xu)):
        with pytest.raises(ValueError):
            tg.log_marginal_likelihood_grid([th], [0.4, 0.5], **kw)
    big = gm.TruncationGP(kernel=RBF(0.2), ratio=0.5, ref=1.0, optimizer=None, backend="cpu")
    big.X_train_, big.y_train_, big.orders_ = X, np.cumsum(np.random.RandomState(2).randn(300, 17), axis=1), np.arange(17)
    with pytest.raises(ValueError, match="at most 15 curves"):
        big.log_marginal_likelihood_grid([th], [0.5], structure="banded")
    # the keyword changes nothing for the routes that were there
    assert gp.log_marginal_likelihood(th, X=X, y=y) == gp.log_marginal_likelihood(th, X=X, y=y, structure=None)
