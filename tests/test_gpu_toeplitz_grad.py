"""The Toeplitz gradient pieces on the device (libgsum_toep.so: k_schur handing out its pivot pairs, k_coeffs, k_levinson, k_diagsums,
k_traces, k_gs_first / k_gs_second, k_tprod, k_hdot): the shared cases of toeplitz_grad_cases.py on backend='hip', and the model layer
at n = 513.  Achieved distances go to the parity record; DESIGN.md section 19."""
import numpy as np
import pytest

from conftest import record_parity

import gsum_amd as gm  # noqa: E402
import toeplitz_cases as tc  # noqa: E402
import toeplitz_grad_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", tc.SIZES)
def test_identities_and_closed_form_inverse_column(n):
    """dt = [t, e_0] on ARFIMA columns, whose every step rotates: trace(t) = n, H(t) = G, trace(e_0) and x against the closed form,
    H(e_0) = alpha^T alpha, T alpha = Z, under the rule of toeplitz_cases against the cpu backend's own distances.  Every size at which
    k_schur and k_levinson change class, the wave and lane edges, and the limit."""
    record_parity(f"toeplitz_grad/identities/n{n}", **gc.check_identities("hip", n))


@pytest.mark.parametrize("name", tc.ill_names())
def test_ill_conditioned_goldens(name):
    """trace, H and alpha against mpmath: at most numpy's dense fp64 route's distance on the same T and within 4 x the cpu backend's."""
    d, d_np, d_cpu = gc.check_golden("hip", name)
    record_parity(f"toeplitz_grad/golden/{name}", trace=d[0], H=d[1], alpha=d[2], numpy_trace=d_np[0], numpy_H=d_np[1], numpy_alpha=d_np[2],
                  cpu_trace=d_cpu[0], cpu_H=d_cpu[1], cpu_alpha=d_cpu[2])


@pytest.mark.parametrize("name", tc.ill_names())
def test_ill_conditioned_goldens_at_double_double_width(name):
    """Double-double on the device against long double on the cpu backend: trace and alpha within 2^-20 of the cpu backend's distance
    (floor 64 * 2^-53), H within that distance.  The check that notices a low word lost where B crosses a thread."""
    gc.check_golden_extended("hip", name)


def test_properties():
    gc.check_properties("hip")


@pytest.mark.parametrize("n", tc.LATE_SIZES)
def test_a_failing_first_column_between_two_good_ones(n):
    record_parity(f"toeplitz_grad/failure_between_good/n{n}", info=gc.check_failure_between_good("hip", n))


def test_first_columns_in_three_launches():
    record_parity("toeplitz_grad/chunk_loop", info=gc.check_chunk_loop("hip"), **gc.CHUNKED)


def test_refusals():
    gc.check_shape_refusals("hip")
    n = gm.toeplitz.toeplitz_max_n("hip") + 1
    t, Z = tc.kms_column(n, 0.5), np.ones((n, 1))
    with pytest.raises(ValueError, match="n must be <= 8192"):
        gm.toeplitz_grad(t, t[None], Z)
    with pytest.raises(ValueError, match="n must be <= 8192"):
        gm.toeplitz_inverse_column(t)
    with pytest.raises(ValueError, match="n must be <= 8192"):
        gm.toeplitz_solve(t, Z)
    t8 = tc.kms_column(8, 0.5)
    for s in (2.0 ** -66, 2.0 ** 66):
        with pytest.raises(ValueError, match=r"t\[0\] must lie within"):
            gm.toeplitz_grad(s * t8, t8[None], np.ones((8, 1)))
        with pytest.raises(ValueError, match=r"t\[0\] must lie within"):
            gm.toeplitz_inverse_column(s * t8)
    for s in (2.0 ** -64, 2.0 ** 64):
        assert gm.toeplitz_grad(s * t8, t8[None], np.ones((8, 1)))[2] == 0 and gm.toeplitz_inverse_column(s * t8)[1] == 0


@pytest.mark.parametrize("name", [c[0] for c in gc.MODEL_CLASSES])
def test_model_gradient_against_long_double_truth(name):
    record_parity(f"toeplitz_grad/model_gradient/{name}_n513", rel=gc.check_model_gradient("hip", name, 513))


@pytest.mark.parametrize("name", [c[0] for c in gc.MODEL_CLASSES])
def test_fit_on_the_structured_route(name, monkeypatch):
    record_parity(f"toeplitz_grad/fit/{name}_n513", value_rel_diff=gc.check_fit("hip", name, 513, monkeypatch))


def test_phase_times_are_reported():
    from gsum_amd import _toep_lib
    h = _toep_lib.default_handle(0)
    h.grad_times(reset=True)
    before = h.times()
    t = tc.arfima_column(300, 0.3)
    gm.toeplitz_grad(t, t[None], np.ones((300, 2)))
    ms = h.grad_times()
    assert tuple(ms) == _toep_lib.GRAD_PHASES and all(v > 0 for v in ms.values())
    assert h.times() == before                                          # the value path's clock is its own
