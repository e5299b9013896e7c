"""The blocked route of the Toeplitz path without a device: the contract of the new entry points of libgsum_toep.so on a fake handle,
``method="blocked"`` in the Python layer, and the cases of toeplitz_blocked_cases.py on backend='cpu', where the keyword selects a
device schedule and therefore nothing: the cpu backend runs its one long-double code.  DESIGN.md section 23."""
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
import toeplitz_panel_cases as pn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsum_toep_blocked_max_n", "gsum_toep_blocked_tile_rows", "gsum_toep_gram_blocked", "gsum_toep_predict_blocked", "gsum_toep_blocked_times")


def test_header_map_prototypes_and_library_agree():
    """include/gsum_toep.h declares and documents each new entry point, the version script exports it, _toep_lib binds it, and the
    built library defines exactly what the header declares."""
    from gsum_amd import _toep_lib, build
    with open(os.path.join(ROOT, "gsum_amd", "csrc", "gsum_toep.map")) as f:
        vmap = f.read()
    with open(os.path.join(ROOT, "include", "gsum_toep.h")) as f:
        header = f.read()
    comment, decls = header.split("#ifndef GSUM_TOEP_H")
    declared = set(re.findall(r"\b(gsum_toep_[a-z0-9_]+)\s*\(", decls))
    assert declared == set(_toep_lib.PROTOTYPES), declared ^ set(_toep_lib.PROTOTYPES)
    out = subprocess.run(["nm", "-D", "--defined-only", build.build_toep()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("gsum_")}
    assert exported == declared
    lib = _toep_lib.load_library()
    for name in NEW:
        assert re.search(r"global:\s*gsum_toep_\*;", vmap) or name in vmap
        assert name in declared and name in comment, name
        assert getattr(lib, name) is not None
    assert "#define GSUM_TOEP_BLOCKED_MAX_N 1048576" in decls
    assert _toep_lib.max_n() == 8192 and _toep_lib.max_n("blocked") == 1048576           # needs no device; the default is unchanged
    assert gm.toeplitz.toeplitz_max_n("cpu", method="blocked") is None
    with pytest.raises(ValueError, match="method must be"):
        gm.toeplitz.toeplitz_max_n("cpu", method="bogus")
    B, R = lib.gsum_toep_panel_width(None), lib.gsum_toep_blocked_tile_rows(None)
    assert R == bk.tile_rows() and R >= 64 and (R + B) % 64 == 0                         # a tile and its halo fill whole waves
    assert _toep_lib.BLOCKED_PHASES == ("h2d", "lead", "tiles", "diag", "update", "sums", "cov", "d2h")
    assert _toep_lib.METHODS == ("columns", "panel", "blocked")


def test_library_refuses_bad_arguments_before_it_touches_a_device():
    """Null pointers, m, n, n_sets < 1, cols and c out of range, n = 1048577, the two 2^31 products and t[0] = 2^+-66 on a null handle
    or a fake one: no device is opened.  The refusals are those of the panel entry points, with the blocked limit on n."""
    from gsum_amd import _toep_lib
    from gsum_amd._sidelib import _d, _i32
    lib = _toep_lib.load_library()
    err = lambda: lib.gsum_toep_last_error().decode()  # noqa: E731
    ptr = lambda a: None if a is None else (_i32(a) if a.dtype == np.int32 else _d(a))  # noqa: E731
    assert lib.gsum_toep_gram_blocked(None, None, 1, 1, None, 1, 1, None, None, None) != 0 and "null pointer" in err()
    assert lib.gsum_toep_predict_blocked(None, None, 1, None, 1, None, 0, None, None, None, None, None, None) != 0 and "null pointer" in err()
    assert lib.gsum_toep_blocked_times(None, None, 0) != 0 and "null pointer" in err()
    assert lib.gsum_toep_blocked_max_n(None) == 1048576
    fake = C_.c_void_p(1)                                               # never dereferenced: every refusal comes first
    t8, big = tc.kms_column(8, 0.5), np.ones(1048577)
    K, Z, out, info = np.ones((8, 2), order="F"), np.ones((8, 17), order="F"), np.zeros(64), np.zeros(1, dtype=np.int32)

    def gram(t=t8, m=1, n=8, Z_=Z, n_sets=1, cols=2, G=out, sld=out, info_=info):
        return lib.gsum_toep_gram_blocked(fake, ptr(t), m, n, ptr(Z_), n_sets, cols, ptr(G), ptr(sld), ptr(info_))

    for missing in (dict(t=None), dict(Z_=None), dict(G=None), dict(sld=None), dict(info_=None)):
        assert gram(**missing) != 0 and "null pointer" in err(), missing
    for zero in (dict(m=0), dict(n=0), dict(n_sets=0)):
        assert gram(**zero) != 0 and "must be >= 1" in err(), zero
    assert gram(cols=17) != 0 and "cols must be between 1 and 16" in err()
    assert gram(cols=0) != 0 and "cols must be between 1 and 16" in err()
    assert gram(t=big, n=1048577) != 0 and "n must be <= 1048576" in err() and "gsum_toep_gram_blocked" in err()
    assert gram(n_sets=2 ** 15, cols=16, n=4096, t=np.ones(4096)) != 0 and "must be < 2^31" in err()      # 4096 * 2^15 * 16 = 2^31
    assert gram(n_sets=128, cols=16, n=1048576, t=big) != 0 and "must be < 2^31" in err()                  # 2^20 * 2^7 * 16 = 2^31
    assert gram(n_sets=65536, cols=1) != 0 and "n_sets must be <= 65535" in err()
    for s in (2.0 ** -66, 2.0 ** 66):
        assert gram(t=s * t8) != 0 and "t[0] must lie within" in err()

    def predict(t=t8, n=8, K_=K, q=2, Z_=Z, c=2, quad=out, cross=out, G=out, sld=out, info_=info):
        return lib.gsum_toep_predict_blocked(fake, ptr(t), n, ptr(K_), q, ptr(Z_), c, ptr(quad), ptr(cross), None, ptr(G), ptr(sld), ptr(info_))

    for missing in (dict(t=None), dict(K_=None), dict(quad=None), dict(sld=None), dict(info_=None), dict(Z_=None), dict(cross=None), dict(G=None)):
        assert predict(**missing) != 0 and "null pointer" in err(), missing
    assert predict(q=0) != 0 and "q must be >= 1" in err()
    assert predict(n=0) != 0 and "must be >= 1" in err()
    assert predict(c=17) != 0 and "c must be between 0 and 16" in err()
    assert predict(c=-1) != 0 and "c must be between 0 and 16" in err()
    assert predict(t=big, n=1048577) != 0 and "n must be <= 1048576" in err() and "gsum_toep_predict_blocked" in err()
    assert predict(q=2 ** 28 - 2) != 0 and "n * (q + c) must be < 2^31" in err()          # 8 (2^28 - 2 + 2) = 2^31
    for s in (2.0 ** -66, 2.0 ** 66):
        assert predict(t=s * t8) != 0 and "t[0] must lie within" in err()
    # the other routes keep their limit
    t9 = np.ones(8193)
    assert lib.gsum_toep_gram_panel(fake, ptr(t9), 1, 8193, ptr(Z), 1, 2, ptr(out), ptr(out), ptr(info)) != 0 and "n must be <= 8192" in err()
    assert lib.gsum_toep_gram(fake, ptr(t9), 1, 8193, ptr(Z), 1, 2, ptr(out), ptr(out), ptr(info)) != 0 and "n must be <= 8192" in err()


def test_method_is_checked():
    from gsum_amd import _toep_lib
    assert _toep_lib.check_method("blocked") == "blocked" and _toep_lib.check_method("blocked", "toeplitz_method") == "blocked"
    t, Z = tc.kms_column(8, 0.5), np.ones((8, 2))
    for bad in ("bogus", None, "Blocked"):
        with pytest.raises(ValueError, match='method must be "columns" or "panel" or "blocked"'):
            _toep_lib.check_method(bad)
        with pytest.raises(ValueError, match='method must be "columns" or "panel"'):
            gm.toeplitz_gram(t, Z, backend="cpu", method=bad)
        with pytest.raises(ValueError, match='method must be "columns" or "panel"'):
            gm.toeplitz_predict(t, Z, backend="cpu", method=bad)
    with pytest.raises(ValueError, match='toeplitz_method must be "columns" or "panel" or "blocked"'):
        _toep_lib.check_method("bogus", "toeplitz_method")


@pytest.mark.parametrize("n", (1, 2, 17, 129, 513))
def test_cpu_backend_gives_the_same_bits_for_every_method(n):
    """The keyword selects a device schedule, not an arithmetic."""
    t = pn.arfima_columns(n)
    Z = tc.rhs_columns(n, 6)
    a, b, c = (gm.toeplitz_gram(t, Z, 2, backend="cpu", method=m) for m in ("blocked", "panel", "columns"))
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c))
    K = tc.rhs_columns(n, 5, seed=1)
    p, q, r = (gm.toeplitz_predict(t[0], K, Z[:, :2], want_cov=True, backend="cpu", method=m) for m in ("blocked", "panel", "columns"))
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(p, q, r))


def test_cases_on_the_cpu_backend():
    bk.check_equal_to_panel("cpu", 2 * bk.width() + 1, 17)
    bk.check_predict_equal_to_panel("cpu", 129)
    bk.check_ill_equal_to_panel("cpu", "matern52_n64")
    bk.check_independence("cpu", 129)
    bk.check_late_failures("cpu", bk.tile_rows() + bk.width() + 5)


def test_the_chunked_shape_crosses_the_budget_by_one_first_column():
    n = 8192 + bk.tile_rows() + 1
    c, n_sets, m = bk.chunked_shape(n)
    assert bk.first_columns_per_launch(n, n_sets * c, m) == 2 and bk.first_columns_per_launch(n, (n_sets - 1) * c, m) == 3
    assert n * n_sets * c < 2 ** 31 and n_sets <= 65535


def test_the_golden_is_what_its_generator_describes():
    g = bk.blocked_golden()
    assert g["digits"] == 60 and [c["d"] for c in g["arfima"]] == list(tc.DS)
    for c in g["arfima"]:
        assert c["n"] == 8193 and c["cols"] == 4 and np.array(c["G"]).shape == (4, 4)
        # the fp64 column's sum_log_diag against the closed form of the unrounded column: the rounding of t moves it by a few eps
        assert abs(c["sum_log_diag"] - tc.arfima_sum_log_diag(8193, c["d"])) <= tc.FLOOR * abs(c["sum_log_diag"])
        assert abs(c["sum_log_diag_closed_form"] - tc.arfima_sum_log_diag(8193, c["d"])) <= 4 * tc.EPS * abs(c["sum_log_diag"])


def test_surface():
    bk.check_surface("cpu", 40)


@pytest.mark.parametrize("name", [c[0] for c in gc.MODEL_CLASSES])
def test_model_layer(name):
    bk.check_model("cpu", name, 40)
