"""The blocked route of the Toeplitz path on the device (libgsum_toep.so: k_blocked_init, k_schur_lead, k_schur_tiles, k_blocked_sld, then
the panel route's k_panel_diag and k_panel_update): the cases of toeplitz_blocked_cases.py on backend='hip'.  Every test passes
``method="blocked"`` / ``toeplitz_method="blocked"``.  DESIGN.md section 23."""
import numpy as np
import pytest

from conftest import record_parity

import gsum_amd as gm  # noqa: E402
import toeplitz_blocked_cases as bk  # noqa: E402
import toeplitz_cases as tc  # noqa: E402
import toeplitz_grad_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu


def _beyond():
    return 8192 + bk.tile_rows() + 1


@pytest.mark.parametrize("ncols", bk.COLUMN_COUNTS)
@pytest.mark.parametrize("size", bk.EDGE_SIZES)
def test_bit_equal_to_the_panel_route(size, ncols):
    """(1) Measured on mutated libraries: notices a halo one row short and a skipped last partial tile (every
    n > R), a lead window one row short (every n >= 2) and a low word of v dropped from the state (from n = 2 B + 1 on)."""
    n = bk.edge_size(size)
    record_parity(f"toeplitz_blocked/equal/n{n}_c{ncols}", **bk.check_equal_to_panel("hip", n, ncols))


def test_bit_equal_to_the_panel_route_wide():
    record_parity("toeplitz_blocked/equal/wide", **bk.check_equal_to_panel("hip", 2 * bk.tile_rows() + 17, bk.WIDE))


@pytest.mark.parametrize("size", ("R+B+1", "2049"))
def test_predict_bit_equal_to_the_panel_route(size):
    record_parity(f"toeplitz_blocked/predict_equal/{size}", sld=bk.check_predict_equal_to_panel("hip", bk.edge_size(size)))


@pytest.mark.parametrize("name", tc.ill_names())
def test_ill_conditioned_goldens_bit_equal_to_the_panel_route(name):
    d = bk.check_ill_equal_to_panel("hip", name)
    record_parity(f"toeplitz_blocked/golden/{name}", G=d[0], sld=d[1])


@pytest.mark.parametrize("size", bk.BEYOND_SIZES)
def test_sum_log_diag_beyond_the_limit(size):
    n = bk.beyond_size(size)
    record_parity(f"toeplitz_blocked/sld/n{n}", **bk.check_sum_log_diag("hip", n))


@pytest.mark.parametrize("size", bk.BEYOND_SIZES)
def test_closed_form_beyond_the_limit(size):
    n = bk.beyond_size(size)
    record_parity(f"toeplitz_blocked/kms/n{n}", **bk.check_kms("hip", n))


def test_arfima_golden_beyond_the_limit():
    record_parity("toeplitz_blocked/arfima_golden/n8193", **bk.check_arfima_golden("hip"))


@pytest.mark.parametrize("n", (8193, 16385))
def test_new_points_on_the_training_points_beyond_the_limit(n):
    record_parity(f"toeplitz_blocked/identity/n{n}", **bk.check_identity("hip", n))


def test_independence():
    record_parity("toeplitz_blocked/independence", sld=bk.check_independence("hip", _beyond()))


def test_first_columns_in_two_launches():
    record_parity("toeplitz_blocked/chunk_loop", info=bk.check_chunk_loop("hip", _beyond()))


def test_late_failures():
    record_parity("toeplitz_blocked/late_failures", info=bk.check_late_failures("hip", _beyond()))


def test_other_routes_are_undisturbed_and_their_clocks_are_not_charged():
    record_parity("toeplitz_blocked/clocks", **bk.check_other_routes_undisturbed())


def test_limits_reach_python():
    assert gm.toeplitz.toeplitz_max_n("hip") == 8192 and gm.toeplitz.toeplitz_max_n("hip", method="blocked") == 1048576
    n = 8193
    t = tc.kms_column(n, 0.5)
    for method in ("columns", "panel"):
        with pytest.raises(ValueError, match="n must be <= 8192"):
            gm.toeplitz_gram(t, np.ones((n, 1)), method=method)
    assert gm.toeplitz_gram(t, np.ones((n, 1)), method="blocked")[2] == 0
    for refused in (gm.toeplitz_solve, gm.toeplitz_inverse_column, gm.toeplitz_inverse_diagonal):
        with pytest.raises(ValueError, match="n must be <= 8192"):
            refused(t, np.ones((n, 1))) if refused is gm.toeplitz_solve else refused(t)
    t8 = tc.kms_column(8, 0.5)
    for s in (2.0 ** -66, 2.0 ** 66):
        with pytest.raises(ValueError, match=r"t\[0\] must lie within"):
            gm.toeplitz_gram(s * t8, np.ones((8, 1)), method="blocked")
    for s in (2.0 ** -64, 2.0 ** 64):
        assert gm.toeplitz_gram(s * t8, np.ones((8, 1)), method="blocked")[2] == 0


def test_surface():
    record_parity("toeplitz_blocked/surface_n513", max_lml=bk.check_surface("hip", 513))


@pytest.mark.parametrize("name", [c[0] for c in gc.MODEL_CLASSES])
def test_model_layer(name):
    record_parity(f"toeplitz_blocked/model/{name}_n513", worst_rel_vs_panel=bk.check_model("hip", name, 513))


def test_fit_and_predict_beyond_the_limit():
    d_mean, d_std = bk.check_fit_beyond_the_limit("hip")
    record_parity("toeplitz_blocked/fit_n8193", mean_vs_n8192=d_mean, std_vs_n8192=d_std)


def test_the_gradient_keeps_its_limit():
    """With an optimiser at n = 8193 the calibration's gradient raises its own refusal; nothing falls back."""
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    n = 8193
    X = np.linspace(0, 1, n)[:, None]
    y = np.random.RandomState(1).randn(n, 2)
    gp = gm.ConjugateGaussianProcess(kernel=Matern(0.2, nu=0.5) + WhiteKernel(1e-6, noise_level_bounds="fixed"), backend="hip", center=0.1, disp=1.5,
                                     df=2, scale=0.7)
    with pytest.raises(ValueError, match="n must be <= 8192"):
        gp.fit(X, y, structure="toeplitz", dense_factor=False, toeplitz_method="blocked")
