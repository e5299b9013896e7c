"""The panel route of the Toeplitz path on the device (libgsum_toep.so: k_schur_panel, k_panel_diag, k_panel_update on the fp64 MFMA):
the shared cases of toeplitz_panel_cases.py on backend='hip'.  Every test passes ``method="panel"``.  DESIGN.md section 21.

Measured on an MI355X (B = 64, 128 and 256): G, quad, cross and cov of the panel route were bit-equal to the column route's in every
case below -- the matrix instruction's four-term step rounded like four sequential FMAs -- but the tests hold the two routes to each
other only within the sum of their bounds, as DESIGN.md section 21 explains."""
import numpy as np
import pytest

from conftest import record_parity

import gsum_amd as gm  # noqa: E402
import toeplitz_cases as tc  # noqa: E402
import toeplitz_grad_cases as gc  # noqa: E402
import toeplitz_panel_cases as pn  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ncols", pn.COLUMN_COUNTS)
@pytest.mark.parametrize("size", pn.EDGE_SIZES)
def test_panel_and_tile_edges(size, ncols):
    """n around one MFMA row tile, one panel and two; ncols around one 16-column tile and into the third.  Notices a K loop that
    starts at k0 + 1 and a skipped last partial row tile (n = 2 B + 1, 2 B + 17)."""
    n = pn.edge_size(size)
    out = pn.check_edges("hip", n, ncols)
    record_parity(f"toeplitz_panel/edges/n{n}_c{ncols}", **out)


@pytest.mark.parametrize("n", pn.CLASS_EDGES)
def test_size_class_edges(n):
    """Once each: where k_schur_panel changes its elements per thread, v's LDS home, and the limit.  (On these well-conditioned
    columns a low word of v dropped between panels moves nothing: test_ill_conditioned_goldens[rbf_n2049] is the test for that.)"""
    record_parity(f"toeplitz_panel/class_edges/n{n}", **pn.check_edges("hip", n, 17))


def test_wide_case():
    record_parity("toeplitz_panel/edges/wide", **pn.check_edges("hip", 2 * pn.width() + 17, pn.WIDE))


@pytest.mark.parametrize("n", tc.arfima_golden_sizes())
def test_arfima_goldens(n):
    record_parity(f"toeplitz_panel/arfima_golden/n{n}", **pn.check_arfima_golden("hip", n))


@pytest.mark.parametrize("name", tc.ill_names())
def test_ill_conditioned_goldens(name):
    """All eight first columns through gram: at most numpy's dense Cholesky's distance from the mpmath truth, within 4 x the cpu
    backend's, within 4 x the column route's own distance, and sum_log_diag bit-equal to the column route's.  Measured on mutated
    libraries: with the correction word dropped in the trailing update matern52_n513 sits at 1.0e-12 against the column route's
    3.6e-14 and fails the third bound (the first two, at 9.1e-7 and 1.9e-8, do not see it); with the low word of v dropped from the
    state between panels rbf_n2049's sum_log_diag ends in ...371 instead of ...369 and fails the bit equality."""
    d, d_np, d_cpu = pn.check_ill("hip", name)
    record_parity(f"toeplitz_panel/golden/{name}", G=d[0], sld=d[1], numpy_G=d_np[0], cpu_G=d_cpu[0])


@pytest.mark.parametrize("name", tc.ill_names())
def test_off_grid_goldens(name):
    d, d_np, d_cpu = pn.check_offgrid("hip", name)
    record_parity(f"toeplitz_panel/offgrid_golden/{name}", **{k: d[i] for i, k in enumerate(pn.pc.PIECES)})


@pytest.mark.parametrize("n", (64, 513, 2049, 4097))
def test_new_points_on_the_training_points(n):
    record_parity(f"toeplitz_panel/identity/n{n}", **pn.check_identity("hip", n))


def test_gram_independence():
    pn.check_gram_independence("hip")


def test_predict_independence():
    record_parity("toeplitz_panel/predict_bit_equal_to_columns", equal=pn.check_predict_independence("hip"))


def test_first_columns_in_two_launches():
    info = pn.check_chunk_loop("hip")
    record_parity("toeplitz_panel/chunk_loop", info=info)


def test_column_route_is_undisturbed_and_its_clocks_are_not_charged():
    ms = pn.check_column_route_undisturbed()
    record_parity("toeplitz_panel/clocks", **ms)


@pytest.mark.parametrize("n", (513, 2049))
def test_late_failures(n):
    info = pn.check_late_failures("hip", n)
    record_parity(f"toeplitz_panel/late_failures/n{n}", info=info)


def test_refusals_reach_python():
    n = gm.toeplitz.toeplitz_max_n("hip") + 1
    t = tc.kms_column(n, 0.5)
    with pytest.raises(ValueError, match="n must be <= 8192"):
        gm.toeplitz_gram(t, np.ones((n, 1)), method="panel")
    with pytest.raises(ValueError, match="n must be <= 8192"):
        gm.toeplitz_predict(t, np.ones((n, 2)), method="panel")
    t8 = tc.kms_column(8, 0.5)
    for s in (2.0 ** -66, 2.0 ** 66):
        with pytest.raises(ValueError, match=r"t\[0\] must lie within"):
            gm.toeplitz_gram(s * t8, np.ones((8, 1)), method="panel")
    for s in (2.0 ** -64, 2.0 ** 64):
        assert gm.toeplitz_gram(s * t8, np.ones((8, 1)), method="panel")[2] == 0
    with pytest.raises(ValueError, match="method must be"):
        gm.toeplitz_gram(t8, np.ones((8, 1)), method="bogus")


def test_surface():
    record_parity("toeplitz_panel/surface_n513", max_rel=pn.check_surface("hip", 513))


@pytest.mark.parametrize("name", [c[0] for c in gc.MODEL_CLASSES])
def test_model_layer(name):
    record_parity(f"toeplitz_panel/model/{name}_n513", worst_rel_vs_columns=pn.check_model("hip", name, 513))
