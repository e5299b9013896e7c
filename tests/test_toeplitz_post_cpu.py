"""The posterior pieces of the Toeplitz path on backend='cpu' (numpy.longdouble recursion, fp64 substitution), the model layer on top
and the contract of the new entry points of libgsum_toep.so (no GPU needed).  The shared cases are in toeplitz_post_cases.py; DESIGN.md
section 20."""
import numpy as np
import pytest

import gsum_amd as gm  # noqa: E402
import toeplitz_cases as tc  # noqa: E402
import toeplitz_grad_cases as gc  # noqa: E402
import toeplitz_post_cases as pc  # noqa: E402


@pytest.mark.parametrize("n", tc.SIZES)
def test_new_points_on_the_training_points(n):
    """K = columns of T itself: quad = t_0, cross = rows of Z, cov = T[idx, idx]; G and sum_log_diag are toeplitz_gram's."""
    pc.check_identity("cpu", n)


@pytest.mark.parametrize("name", tc.ill_names())
def test_new_points_on_the_training_points_of_the_goldens(name):
    pc.check_identity_golden("cpu", name)


def test_goldens_cover_the_ill_cases():
    assert pc.golden_names() == [c["name"] for c in sorted(tc.ill_cases(), key=lambda c: (c["n"], c["name"]))]
    for case in pc.golden()["cases"]:
        n = case["n"]
        assert case["q"] == pc.q_class(n) == len(case["s"]) and case["s"] == pc.off_grid_points(n)
        assert np.shape(case["cross"]) == (case["q"], case["cols"]) and np.shape(case["cov"]) == (case["q"], case["q"]) and len(case["p"]) == n
        assert case["method"] == ("dense" if n <= 128 else "recursion")


@pytest.mark.parametrize("name", tc.ill_names())
def test_off_grid_goldens(name):
    pc.check_offgrid("cpu", name)


@pytest.mark.parametrize("n", tc.SIZES)
def test_inverse_diagonal_on_closed_form_columns(n):
    """p against the prefix of the closed-form x, sum p against trace(T^-1), p against its mirror image: the cpu backend itself sits
    within the floor on all three."""
    pc.check_diagonal("cpu", n)
    assert max(pc.diagonal_distances("cpu", n)) <= pc.FLOOR


def test_prefix_formula_is_the_inverse_diagonal():
    """The Gohberg-Semencul prefix itself, against numpy's dense inverse of small well-conditioned cases."""
    from scipy.linalg import toeplitz
    for d in tc.DS:
        for n in (1, 2, 5, 40):
            want = np.diag(np.linalg.inv(toeplitz(tc.arfima_column(n, d))))
            assert np.max(np.abs(pc.prefix_diagonal(gc.arfima_inverse_column(n, d)).astype(float) - want)) <= 1e-13 * np.max(np.abs(want))


@pytest.mark.parametrize("name", tc.ill_names())
def test_inverse_diagonal_goldens(name):
    pc.check_diagonal_golden("cpu", name)


@pytest.mark.parametrize("n", (257, 4097))
def test_properties(n):
    pc.check_properties("cpu", n)


def test_late_failures():
    pc.check_late_failures("cpu")


def test_shape_refusals():
    pc.check_shape_refusals("cpu")


def test_library_refuses_bad_arguments_before_it_touches_a_device():
    """Null pointers, q < 1, c = 17, n above the limit, n (q + c) >= 2^31 and t[0] outside 2^-64 .. 2^64, on a null handle or a fake one:
    no device is opened."""
    import ctypes as C_
    from gsum_amd import _toep_lib
    from gsum_amd._sidelib import _d, _i32
    lib = _toep_lib.load_library()
    err = lambda: lib.gsum_toep_last_error().decode()  # noqa: E731
    assert lib.gsum_toep_predict(None, None, 1, None, 1, None, 0, None, None, None, None, None, None) != 0 and "null pointer" in err()
    assert lib.gsum_toep_loo(None, None, 1, 1, None, 0, None, None, None) != 0 and "null pointer" in err()
    assert lib.gsum_toep_post_times(None, None, 0) != 0 and "null pointer" in err()
    fake = C_.c_void_p(1)                                               # never dereferenced: every refusal comes first
    t8 = tc.kms_column(8, 0.5)
    K, Z, out, info = np.ones((8, 2), order="F"), np.ones((8, 17), order="F"), np.zeros(64), np.zeros(1, dtype=np.int32)

    def predict(t=t8, n=8, K_=K, q=2, Z_=Z, c=2, quad=out, cross=out, G=out, sld=out, info_=info):
        ptr = lambda a: None if a is None else (_i32(a) if a.dtype == np.int32 else _d(a))  # noqa: E731
        return lib.gsum_toep_predict(fake, ptr(t), n, ptr(K_), q, ptr(Z_), c, ptr(quad), ptr(cross), None, ptr(G), ptr(sld), ptr(info_))

    for missing in (dict(t=None), dict(K_=None), dict(quad=None), dict(sld=None), dict(info_=None), dict(Z_=None), dict(cross=None), dict(G=None)):
        assert predict(**missing) != 0 and "null pointer" in err(), missing
    assert predict(q=0) != 0 and "q must be >= 1" in err()
    assert predict(c=17) != 0 and "c must be between 0 and 16" in err()
    assert predict(c=-1) != 0 and "c must be between 0 and 16" in err()
    big = np.ones(8193)
    assert predict(t=big, n=8193) != 0 and "n must be <= 8192" in err()
    assert predict(q=2 ** 28 - 2) != 0 and "n * (q + c) must be < 2^31" in err()          # 8 (2^28 - 2 + 2) = 2^31
    for s in (2.0 ** -66, 2.0 ** 66):
        assert predict(t=s * t8) != 0 and "t[0] must lie within" in err()
        assert lib.gsum_toep_loo(fake, _d(s * t8), 1, 8, None, 0, _d(out), None, _i32(info)) != 0 and "t[0] must lie within" in err()
    assert lib.gsum_toep_loo(fake, _d(t8), 1, 8, None, 0, None, None, _i32(info)) != 0 and "null pointer" in err()      # p_out may not be NULL
    assert lib.gsum_toep_loo(fake, _d(t8), 1, 8, None, 1, _d(out), _d(out), _i32(info)) != 0 and "null pointer" in err()  # alpha without Z
    assert lib.gsum_toep_loo(fake, _d(big), 1, 8193, None, 0, _d(big), None, _i32(info)) != 0 and "n must be <= 8192" in err()
    assert _toep_lib.POST_PHASES == ("h2d", "schur", "levinson", "sums", "cov", "solve", "d2h")
    for name in ("toeplitz_predict", "toeplitz_inverse_diagonal", "toeplitz_loo"):
        assert name in gm.__all__ and hasattr(gm, name)


@pytest.mark.parametrize("n", (40, 513))
def test_leave_one_out_against_brute_force(n):
    pc.check_loo("cpu", n)


@pytest.mark.parametrize("name", [c[0] for c in gc.MODEL_CLASSES])
def test_model_layer_without_a_dense_factor(name, monkeypatch):
    pc.check_model("cpu", name, 40, monkeypatch)
