"""The posterior pieces of the Toeplitz path on the device (libgsum_toep.so: k_schur's substitution on [K | Z], k_pred_sums, k_pred_cov on
the fp64 MFMA, k_invdiag after k_levinson): the shared cases of toeplitz_post_cases.py on backend='hip', and the model layer at n = 513.
Achieved distances go to the parity record; DESIGN.md section 20."""
import numpy as np
import pytest

from conftest import record_parity

import gsum_amd as gm  # noqa: E402
import toeplitz_cases as tc  # noqa: E402
import toeplitz_grad_cases as gc  # noqa: E402
import toeplitz_post_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", tc.SIZES)
def test_new_points_on_the_training_points(n):
    """K = columns of T itself, q = 2 C + 1 of them (fewer below that): every size class, both halves of every chunk of k_schur, v's LDS
    home, and k_pred_cov's edge tiles at q = 1, 2, 3, 4, 7, 11, 25 and 33."""
    record_parity(f"toeplitz_post/identity/n{n}", **pc.check_identity("hip", n))


@pytest.mark.parametrize("name", tc.ill_names())
def test_new_points_on_the_training_points_of_the_goldens(name):
    d, d_np, d_cpu = pc.check_identity_golden("hip", name)
    record_parity(f"toeplitz_post/identity_golden/{name}", **{k: d[i] for i, k in enumerate(pc.PIECES)},
                  **{"numpy_" + k: d_np[i] for i, k in enumerate(pc.PIECES)}, **{"cpu_" + k: d_cpu[i] for i, k in enumerate(pc.PIECES)})


@pytest.mark.parametrize("name", tc.ill_names())
def test_off_grid_goldens(name):
    """quad, cross and cov of columns that are no kernel build against mpmath: at most numpy's dense fp64 route's distance on the same T
    and within 4 x the cpu backend's."""
    d, d_np, d_cpu = pc.check_offgrid("hip", name)
    record_parity(f"toeplitz_post/offgrid_golden/{name}", **{k: d[i] for i, k in enumerate(pc.PIECES)},
                  **{"numpy_" + k: d_np[i] for i, k in enumerate(pc.PIECES)}, **{"cpu_" + k: d_cpu[i] for i, k in enumerate(pc.PIECES)})


@pytest.mark.parametrize("n", tc.SIZES)
def test_inverse_diagonal_on_closed_form_columns(n):
    record_parity(f"toeplitz_post/diagonal/n{n}", **pc.check_diagonal("hip", n))


@pytest.mark.parametrize("name", tc.ill_names())
def test_inverse_diagonal_goldens(name):
    d, d_np, d_cpu = pc.check_diagonal_golden("hip", name)
    record_parity(f"toeplitz_post/diagonal_golden/{name}", p=d, numpy_p=d_np, cpu_p=d_cpu)


@pytest.mark.parametrize("name", tc.ill_names())
def test_inverse_diagonal_goldens_at_double_double_width(name):
    """Double-double on the device against long double on the cpu backend: p within 2^-20 of the cpu backend's distance (floor
    64 * 2^-53).  The check that notices a lost low word."""
    pc.check_diagonal_golden_extended("hip", name)


@pytest.mark.parametrize("n", (257, 4097))
def test_properties(n):
    pc.check_properties("hip", n)


def test_late_failures():
    record_parity("toeplitz_post/late_failures/n513", info=pc.check_late_failures("hip"))


def test_refusals():
    pc.check_shape_refusals("hip")
    n = gm.toeplitz.toeplitz_max_n("hip") + 1
    t = tc.kms_column(n, 0.5)
    with pytest.raises(ValueError, match="n must be <= 8192"):
        gm.toeplitz_predict(t, np.ones((n, 2)), np.ones((n, 1)))
    with pytest.raises(ValueError, match="n must be <= 8192"):
        gm.toeplitz_inverse_diagonal(t)
    with pytest.raises(ValueError, match="n must be <= 8192"):
        gm.toeplitz_loo(t, np.ones(n))
    t8 = tc.kms_column(8, 0.5)
    for s in (2.0 ** -66, 2.0 ** 66):
        with pytest.raises(ValueError, match=r"t\[0\] must lie within"):
            gm.toeplitz_predict(s * t8, np.ones((8, 2)))
        with pytest.raises(ValueError, match=r"t\[0\] must lie within"):
            gm.toeplitz_inverse_diagonal(s * t8)
    for s in (2.0 ** -64, 2.0 ** 64):
        assert gm.toeplitz_predict(s * t8, np.ones((8, 2))).info == 0 and gm.toeplitz_inverse_diagonal(s * t8)[1] == 0


@pytest.mark.parametrize("n", (65, 513, 2049))
def test_leave_one_out_against_brute_force(n):
    record_parity(f"toeplitz_post/loo/n{n}", **pc.check_loo("hip", n))


@pytest.mark.parametrize("name", [c[0] for c in gc.MODEL_CLASSES])
def test_model_layer_without_a_dense_factor(name, monkeypatch):
    record_parity(f"toeplitz_post/model/{name}_n513", **pc.check_model("hip", name, 513, monkeypatch))
