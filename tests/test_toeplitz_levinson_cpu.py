"""The tiled Levinson replay of the Toeplitz path without a device: a long-double model of k_levinson_tiles' geometry against the
straight recursion, the contract of the new entry points of libgsum_toep.so on a fake handle, and ``method="blocked"`` /
``toeplitz_grad_method="blocked"`` in the Python layer on backend='cpu', where the keyword selects a device schedule and therefore
nothing.  DESIGN.md section 24."""
import ctypes as C_
import os
import re
import subprocess

import numpy as np
import pytest

import gsum_amd as gm  # noqa: E402
import toeplitz_blocked_cases as bk  # noqa: E402
import toeplitz_cases as tc  # noqa: E402
import toeplitz_grad_cases as gc  # noqa: E402
import toeplitz_levinson_cases as lv  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsum_toep_grad_blocked", "gsum_toep_solve_blocked", "gsum_toep_loo_blocked", "gsum_toep_levinson_times")


@pytest.mark.parametrize("size", lv.MODEL_SIZES)
def test_model_of_the_tiled_replay_at_the_library_geometry(size):
    B, R = bk.width(), bk.tile_rows()
    lv.check_model(lv.model_size(size, B, R), B, R)


@pytest.mark.parametrize("geometry", lv.SMALL_GEOMETRIES)
def test_model_of_the_tiled_replay_at_small_geometries(geometry):
    for size in lv.MODEL_SIZES:
        lv.check_model(max(1, lv.model_size(size, *geometry)), *geometry)


@pytest.mark.parametrize("geometry", lv.SMALL_GEOMETRIES + (None,))
@pytest.mark.parametrize("size", ("R+B+1", "2R+17"))
def test_a_wrong_model_is_noticed(size, geometry):
    B, R = geometry or (bk.width(), bk.tile_rows())
    lv.check_model_variants_differ(lv.model_size(size, B, R), B, R)


def test_header_map_prototypes_and_library_agree():
    """include/gsum_toep.h declares and documents each new entry point, the version script exports it, _toep_lib binds it, and the
    built library defines it."""
    from gsum_amd import _toep_lib, build
    with open(os.path.join(ROOT, "gsum_amd", "csrc", "gsum_toep.map")) as f:
        vmap = f.read()
    with open(os.path.join(ROOT, "include", "gsum_toep.h")) as f:
        comment, decls = f.read().split("#ifndef GSUM_TOEP_H")
    declared = set(re.findall(r"\b(gsum_toep_[a-z0-9_]+)\s*\(", decls))
    out = subprocess.run(["nm", "-D", "--defined-only", build.build_toep()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("gsum_")}
    lib = _toep_lib.load_library()
    for name in NEW:
        assert re.search(r"global:\s*gsum_toep_\*;", vmap) or name in vmap
        assert name in declared and name in comment and name in exported and name in _toep_lib.PROTOTYPES, name
        assert getattr(lib, name) is not None
    assert _toep_lib.LEVINSON_PHASES == ("h2d", "lead", "tiles", "diag", "update", "levinson", "gram", "diagsums", "solve", "contract", "d2h")
    assert _toep_lib.GRAD_METHODS == ("columns", "blocked")
    for old, new in (("gsum_toep_grad", "gsum_toep_grad_blocked"), ("gsum_toep_solve", "gsum_toep_solve_blocked"), ("gsum_toep_loo", "gsum_toep_loo_blocked"),
                     ("gsum_toep_blocked_times", "gsum_toep_levinson_times")):
        assert _toep_lib.PROTOTYPES[old] == _toep_lib.PROTOTYPES[new], new                # the arguments of the entry point it follows


def test_library_refuses_bad_arguments_before_it_touches_a_device():
    """Null pointers, P, cols, sets, m, n < 1, n = 1048577, the 2^31 products and t[0] = 2^+-66 on a null handle or a fake one: no device
    is opened.  The refusals are those of gsum_toep_grad, gsum_toep_solve and gsum_toep_loo, with the blocked limit on n; the old entry
    points still refuse 8193."""
    from gsum_amd import _toep_lib
    from gsum_amd._sidelib import _d, _i32
    lib = _toep_lib.load_library()
    err = lambda: lib.gsum_toep_last_error().decode()  # noqa: E731
    ptr = lambda a: None if a is None else (_i32(a) if a.dtype == np.int32 else _d(a))  # noqa: E731
    assert lib.gsum_toep_grad_blocked(None, None, 1, 1, None, 1, None, 1, 1, None, None, None, None, None) != 0 and "null pointer" in err()
    assert lib.gsum_toep_solve_blocked(None, None, 1, 1, None, 1, None, None, None) != 0 and "null pointer" in err()
    assert lib.gsum_toep_loo_blocked(None, None, 1, 1, None, 1, None, None, None) != 0 and "null pointer" in err()
    assert lib.gsum_toep_levinson_times(None, None, 0) != 0 and "null pointer" in err()
    fake = C_.c_void_p(1)                                               # never dereferenced: every refusal comes first
    t8, big, t9 = tc.kms_column(8, 0.5), np.ones(1048577), np.ones(8193)
    Z, out, info = np.ones((8, 17), order="F"), np.zeros(64), np.zeros(1, dtype=np.int32)

    def grad(fn="gsum_toep_grad_blocked", t=t8, m=1, n=8, dt=t8, P=1, Z_=Z, n_sets=1, cols=2, G=out, sld=out, info_=info, trace=out, H=out):
        return getattr(lib, fn)(fake, ptr(t), m, n, ptr(dt), P, ptr(Z_), n_sets, cols, ptr(G), ptr(sld), ptr(info_), ptr(trace), ptr(H))

    for missing in (dict(t=None), dict(dt=None), dict(Z_=None), dict(G=None), dict(sld=None), dict(info_=None), dict(trace=None), dict(H=None)):
        assert grad(**missing) != 0 and "gsum_toep_grad_blocked: null pointer" in err(), missing
    for zero in (dict(m=0), dict(n=0), dict(n_sets=0)):
        assert grad(**zero) != 0 and "must be >= 1" in err(), zero
    for P in (0, 65536):
        assert grad(P=P) != 0 and "P must be between 1 and 65535" in err()
    for cols in (0, 17):
        assert grad(cols=cols) != 0 and "cols must be between 1 and 16" in err()
    assert grad(t=big, n=1048577) != 0 and "n must be <= 1048576" in err() and "gsum_toep_grad_blocked" in err()
    assert grad(n_sets=2 ** 15, cols=16, n=4096, t=np.ones(4096)) != 0 and "must be < 2^31" in err()
    assert grad(n_sets=128, cols=16, n=1048576, t=big) != 0 and "must be < 2^31" in err()
    assert grad(n_sets=65536, cols=1) != 0 and "n_sets must be <= 65535" in err()
    for s in (2.0 ** -66, 2.0 ** 66):
        assert grad(t=s * t8) != 0 and "t[0] must lie within" in err()

    def solve(fn, t=t8, m=1, n=8, Z_=Z, ncols=2, first=out, alpha=out, info_=info):
        return getattr(lib, fn)(fake, ptr(t), m, n, ptr(Z_), ncols, ptr(first), ptr(alpha), ptr(info_))

    for fn in ("gsum_toep_solve_blocked", "gsum_toep_loo_blocked"):
        for missing in (dict(t=None), dict(info_=None), dict(Z_=None), dict(first=None, alpha=None)):
            assert solve(fn, **missing) != 0 and fn + ": null pointer" in err(), (fn, missing)
        for zero in (dict(m=0), dict(n=0)):
            assert solve(fn, **zero) != 0 and "must be >= 1" in err(), (fn, zero)
        assert solve(fn, ncols=0) != 0 and "ncols must be >= 1" in err()
        assert solve(fn, t=big, n=1048577) != 0 and "n must be <= 1048576" in err() and fn in err()
        assert solve(fn, ncols=2 ** 28) != 0 and "n * ncols must be < 2^31" in err()
        for s in (2.0 ** -66, 2.0 ** 66):
            assert solve(fn, t=s * t8) != 0 and "t[0] must lie within" in err()
    assert solve("gsum_toep_loo_blocked", first=None) != 0 and "null pointer" in err()
    # the entry points they follow keep their limit and their text
    assert grad("gsum_toep_grad", t=t9, n=8193, dt=t9) != 0 and "gsum_toep_grad: n must be <= 8192 (one workgroup holds the generator), got 8193" == err()
    for fn in ("gsum_toep_solve", "gsum_toep_loo"):
        assert solve(fn, t=t9, n=8193) != 0 and fn + ": n must be <= 8192 (one workgroup holds the generator), got 8193" == err()


def test_method_is_checked():
    from gsum_amd import _toep_lib
    assert _toep_lib.check_grad_method("blocked") == "blocked" and _toep_lib.check_grad_method("columns", "toeplitz_grad_method") == "columns"
    t, Z = tc.kms_column(8, 0.5), np.ones((8, 2))
    calls = (lambda m: gm.toeplitz_grad(t, t[None], Z, backend="cpu", method=m), lambda m: gm.toeplitz_solve(t, Z, backend="cpu", method=m),
             lambda m: gm.toeplitz_inverse_column(t, backend="cpu", method=m), lambda m: gm.toeplitz_inverse_diagonal(t, backend="cpu", method=m),
             lambda m: gm.toeplitz_loo(t, Z, backend="cpu", method=m))
    for bad in ("panel", "bogus", None, "Blocked"):
        for call in calls:
            with pytest.raises(ValueError, match='method must be "columns" or "blocked"'):
                call(bad)
    gp = gc.model_process(gm.ConjugateGaussianProcess, "cpu", optimizer=None, **dict(gc.MODEL_CLASSES)["gaussian"])
    X, y = gc.model_xy(40)
    with pytest.raises(ValueError, match='toeplitz_grad_method must be "columns" or "blocked"'):
        gp.log_marginal_likelihood_batch([gc.MODEL_THETAS[0]], X=X, y=y, structure="toeplitz", eval_gradient=True, toeplitz_grad_method="panel")
    with pytest.raises(ValueError, match='toeplitz_grad_method must be "columns" or "blocked"'):
        gp.fit(X, y, structure="toeplitz", toeplitz_grad_method="panel")
    gp.fit(X, y, structure="toeplitz", dense_factor=False)
    with pytest.raises(ValueError, match='toeplitz_method must be "columns" or "blocked"'):
        gp.loo(toeplitz_method="panel")


@pytest.mark.parametrize("n", (1, 2, 17, 129, 513))
def test_cpu_backend_gives_the_same_bits_for_both_methods(n):
    """The keyword selects a device schedule, not an arithmetic."""
    t = bk.pn.arfima_columns(n)
    dt = np.stack([np.stack([ti, np.cos(np.arange(n))]) for ti in t])
    Z = tc.rhs_columns(n, 3)
    a, b = (lv.all_pieces(t, dt, Z, "cpu", m) for m in ("blocked", "columns"))
    assert lv._same(a, b)
    la, lb = (gm.toeplitz_loo(t[0], Z, 0.25, backend="cpu", method=m) for m in ("blocked", "columns"))
    assert lv._same(la, lb)


def test_cases_on_the_cpu_backend():
    lv.check_equal_to_columns("cpu", 2 * bk.width() + 1)
    lv.check_golden_equal_to_columns("cpu", "matern52_n64")
    lv.check_independence("cpu", 129)
    lv.check_failures("cpu", bk.tile_rows() + bk.width() + 5)


def test_the_chunked_shape_crosses_the_budget_by_one_first_column():
    n = 8192 + bk.tile_rows() + 1
    n_sets = lv.chunked_sets(n)
    assert lv.first_columns_per_launch(n, n_sets * 16, 1, 3) == 2 and lv.first_columns_per_launch(n, (n_sets - 1) * 16, 1, 3) == 3
    assert n * n_sets * 16 < 2 ** 31 and n_sets <= 65535


@pytest.mark.parametrize("name", [c[0] for c in gc.MODEL_CLASSES])
def test_model_layer(name):
    """toeplitz_grad_method="blocked" on the model classes at n = 40: the batch with its gradients, a fit with the default optimiser
    and the lock-step restarts, and loo, each array-equal to the default."""
    col, blk, vals = lv.check_model_gradient_equal("cpu", name, 40)
    assert lv._grads_equal(col, blk) and [v[0] for v in blk] == list(vals)
    cls, kw = gc.model_class(name), dict(gc.MODEL_CLASSES)[name]
    X, y = gc.model_xy(40)
    for restarts in (0, 2):
        fits = [gc.model_process(cls, "cpu", n_restarts_optimizer=restarts, random_state=5, **kw).fit(X, y, structure="toeplitz", toeplitz_grad_method=m)
                for m in ("blocked", "columns")]
        assert np.array_equal(fits[0].kernel_.theta, fits[1].kernel_.theta)
        assert fits[0].log_marginal_likelihood_value_ == fits[1].log_marginal_likelihood_value_
    if name == "gaussian":
        gp = gc.model_process(cls, "cpu", **kw).fit(X, y, structure="toeplitz", dense_factor=False, toeplitz_method="blocked", toeplitz_grad_method="blocked")
        assert lv._same(gp.loo(), gp.loo(toeplitz_method="columns")) and lv._same(gp.loo(), gp.loo(toeplitz_method="blocked"))


def test_the_truncation_classes_pass_the_keyword_down(monkeypatch):
    seen = []
    real = gm.ConjugateGaussianProcess.fit

    def spy(self, *a, **k):
        seen.append(k.get("toeplitz_grad_method"))
        return real(self, *a, **k)

    monkeypatch.setattr(gm.ConjugateGaussianProcess, "fit", spy)
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel
    X = np.linspace(0, 1, 12)[:, None]
    y = np.stack([np.cos(3 * X[:, 0]) * 0.5 ** k for k in range(3)], axis=1).cumsum(axis=1)
    for cls in (gm.TruncationGP, gm.TruncationTP):
        gp = cls(kernel=RBF(0.3) + WhiteKernel(1e-6, noise_level_bounds="fixed"), ref=1.0, ratio=0.5, backend="cpu")
        gp.fit(X, y, orders=np.arange(3), structure="toeplitz", toeplitz_grad_method="blocked")
    assert seen == ["blocked", "blocked"], seen
