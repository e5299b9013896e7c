"""The panel route of the Toeplitz path without a device: the contract of the new entry points of libgsum_toep.so on a fake handle,
``method=`` in the Python layer, and the shared cases of toeplitz_panel_cases.py on backend='cpu', where ``method="panel"`` selects a
device schedule and therefore nothing: the cpu backend runs its one long-double code.  DESIGN.md section 21."""
import ctypes as C_
import os
import re

import numpy as np
import pytest

import gsum_amd as gm  # noqa: E402
import toeplitz_cases as tc  # noqa: E402
import toeplitz_grad_cases as gc  # noqa: E402
import toeplitz_panel_cases as pn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsum_toep_panel_width", "gsum_toep_gram_panel", "gsum_toep_predict_panel", "gsum_toep_panel_times")


def test_library_refuses_bad_arguments_before_it_touches_a_device():
    """Null pointers, n = 8193, q < 1, c = 17, cols = 17, n * ncols >= 2^31 and t[0] = 2^+-66 on a null handle or a fake one: no device
    is opened.  The refusals are those of gsum_toep_gram and gsum_toep_predict."""
    from gsum_amd import _toep_lib
    from gsum_amd._sidelib import _d, _i32
    lib = _toep_lib.load_library()
    err = lambda: lib.gsum_toep_last_error().decode()  # noqa: E731
    ptr = lambda a: None if a is None else (_i32(a) if a.dtype == np.int32 else _d(a))  # noqa: E731
    assert lib.gsum_toep_gram_panel(None, None, 1, 1, None, 1, 1, None, None, None) != 0 and "null pointer" in err()
    assert lib.gsum_toep_predict_panel(None, None, 1, None, 1, None, 0, None, None, None, None, None, None) != 0 and "null pointer" in err()
    assert lib.gsum_toep_panel_times(None, None, 0) != 0 and "null pointer" in err()
    B = lib.gsum_toep_panel_width(None)
    assert B == gm.toeplitz_panel_width() and 64 <= B <= 256 and B % 16 == 0
    fake = C_.c_void_p(1)                                               # never dereferenced: every refusal comes first
    t8, big = tc.kms_column(8, 0.5), np.ones(8193)
    K, Z, out, info = np.ones((8, 2), order="F"), np.ones((8, 17), order="F"), np.zeros(64), np.zeros(1, dtype=np.int32)

    def gram(t=t8, m=1, n=8, Z_=Z, n_sets=1, cols=2, G=out, sld=out, info_=info):
        return lib.gsum_toep_gram_panel(fake, ptr(t), m, n, ptr(Z_), n_sets, cols, ptr(G), ptr(sld), ptr(info_))

    for missing in (dict(t=None), dict(Z_=None), dict(G=None), dict(sld=None), dict(info_=None)):
        assert gram(**missing) != 0 and "null pointer" in err(), missing
    for zero in (dict(m=0), dict(n=0), dict(n_sets=0)):
        assert gram(**zero) != 0 and "must be >= 1" in err(), zero
    assert gram(cols=17) != 0 and "cols must be between 1 and 16" in err()
    assert gram(cols=0) != 0 and "cols must be between 1 and 16" in err()
    assert gram(t=big, n=8193) != 0 and "n must be <= 8192" in err()
    assert gram(n_sets=2 ** 15, cols=16, n=4096, t=np.ones(4096)) != 0 and "must be < 2^31" in err()      # 4096 * 2^15 * 16 = 2^31
    assert gram(n_sets=65536, cols=1) != 0 and "n_sets must be <= 65535" in err()
    for s in (2.0 ** -66, 2.0 ** 66):
        assert gram(t=s * t8) != 0 and "t[0] must lie within" in err()

    def predict(t=t8, n=8, K_=K, q=2, Z_=Z, c=2, quad=out, cross=out, G=out, sld=out, info_=info):
        return lib.gsum_toep_predict_panel(fake, ptr(t), n, ptr(K_), q, ptr(Z_), c, ptr(quad), ptr(cross), None, ptr(G), ptr(sld), ptr(info_))

    for missing in (dict(t=None), dict(K_=None), dict(quad=None), dict(sld=None), dict(info_=None), dict(Z_=None), dict(cross=None), dict(G=None)):
        assert predict(**missing) != 0 and "null pointer" in err(), missing
    assert predict(q=0) != 0 and "q must be >= 1" in err()
    assert predict(c=17) != 0 and "c must be between 0 and 16" in err()
    assert predict(c=-1) != 0 and "c must be between 0 and 16" in err()
    assert predict(t=big, n=8193) != 0 and "n must be <= 8192" in err()
    assert predict(q=2 ** 28 - 2) != 0 and "n * (q + c) must be < 2^31" in err()          # 8 (2^28 - 2 + 2) = 2^31
    for s in (2.0 ** -66, 2.0 ** 66):
        assert predict(t=s * t8) != 0 and "t[0] must lie within" in err()
    assert _toep_lib.PANEL_PHASES == ("h2d", "recursion", "diag", "update", "sums", "cov", "d2h")
    assert "toeplitz_panel_width" in gm.__all__ and hasattr(gm, "toeplitz_panel_width")


def test_new_symbols_are_in_the_map_and_the_header():
    """The version script exports gsum_toep_* and nothing else, and the header declares and documents each new entry point."""
    with open(os.path.join(ROOT, "gsum_amd", "csrc", "gsum_toep.map")) as f:
        vmap = f.read()
    with open(os.path.join(ROOT, "include", "gsum_toep.h")) as f:
        header = f.read()
    comment, decls = header.split("#ifndef GSUM_TOEP_H")
    from gsum_amd import _toep_lib
    lib = _toep_lib.load_library()
    for name in NEW:
        assert re.search(r"global:\s*gsum_toep_\*;", vmap) or name in vmap
        assert re.search(r"\b" + name + r"\(", decls), name
        assert name in comment, name
        assert name in _toep_lib.PROTOTYPES and getattr(lib, name) is not None


def test_method_is_checked_on_either_backend():
    t, Z = tc.kms_column(8, 0.5), np.ones((8, 2))
    for bad in ("bogus", None, "Panel"):
        with pytest.raises(ValueError, match='method must be "columns" or "panel"'):
            gm.toeplitz_gram(t, Z, backend="cpu", method=bad)
        with pytest.raises(ValueError, match='method must be "columns" or "panel"'):
            gm.toeplitz_predict(t, Z, backend="cpu", method=bad)
    from gsum_amd import _toep_lib
    with pytest.raises(ValueError, match='method must be "columns" or "panel"'):
        _toep_lib.check_method("bogus")


@pytest.mark.parametrize("n", (1, 2, 17, 129, 513))
def test_cpu_backend_gives_the_same_bits_for_either_method(n):
    """The keyword selects a device schedule, not an arithmetic."""
    t = pn.arfima_columns(n)
    Z = tc.rhs_columns(n, 6)
    a, b = gm.toeplitz_gram(t, Z, 2, backend="cpu", method="panel"), gm.toeplitz_gram(t, Z, 2, backend="cpu", method="columns")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    K = tc.rhs_columns(n, 5, seed=1)
    p, c = (gm.toeplitz_predict(t[0], K, Z[:, :2], want_cov=True, backend="cpu", method=m) for m in ("panel", "columns"))
    assert all(np.array_equal(x, y) for x, y in zip(p, c))


@pytest.mark.parametrize("ncols", pn.COLUMN_COUNTS)
def test_edges(ncols):
    for n in (1, 2, 17, pn.width() + 1, 2 * pn.width() + 17):
        pn.check_edges("cpu", n, ncols)


def test_properties_and_failures():
    pn.check_gram_independence("cpu")
    pn.check_predict_independence("cpu")
    pn.check_late_failures("cpu", 513)


def test_the_chunked_shape_crosses_the_budget_by_one_first_column():
    n, c, n_sets, m = pn.chunked_shape()
    assert pn.first_columns_per_launch(n, n_sets * c, m) == 2 and pn.first_columns_per_launch(n, n_sets * c // 2, m) == 3
    assert n * n_sets * c < 2 ** 31 and n_sets <= 65535


@pytest.mark.parametrize("name", ("matern52_n64", "rbf_n128"))
def test_goldens(name):
    pn.check_ill("cpu", name)
    pn.check_offgrid("cpu", name)


def test_surface():
    pn.check_surface("cpu", 40)


@pytest.mark.parametrize("name", [c[0] for c in gc.MODEL_CLASSES])
def test_model_layer(name):
    pn.check_model("cpu", name, 40)
