"""The tiled Levinson replay of the Toeplitz path on the device (libgsum_toep.so: the blocked route's recursion with its coefficients
kept, k_levinson_tiles, k_levinson_finish, k_invdiag_n, then the kernels of gsum_toep_grad from x on): the cases of
toeplitz_levinson_cases.py on backend='hip'.  Every test passes ``method="blocked"`` / ``toeplitz_grad_method="blocked"``.
DESIGN.md section 24."""
import numpy as np
import pytest

from conftest import record_parity

import gsum_amd as gm  # noqa: E402
import toeplitz_blocked_cases as bk  # noqa: E402
import toeplitz_cases as tc  # noqa: E402
import toeplitz_grad_cases as gc  # noqa: E402
import toeplitz_levinson_cases as lv  # noqa: E402

pytestmark = pytest.mark.gpu


def _beyond():
    return 8192 + bk.tile_rows() + 1


@pytest.mark.parametrize("size", bk.EDGE_SIZES)
def test_bit_equal_to_the_default_method(size):
    """(1) What this notices on mutated libraries is in DESIGN.md section 24."""
    n = bk.edge_size(size)
    record_parity(f"toeplitz_levinson/equal/n{n}", **lv.check_equal_to_columns("hip", n))


@pytest.mark.parametrize("name", gc.golden_names())
def test_ill_conditioned_goldens_bit_equal_to_the_default_method(name):
    record_parity(f"toeplitz_levinson/golden/{name}", trace=lv.check_golden_equal_to_columns("hip", name))


@pytest.mark.parametrize("size", bk.BEYOND_SIZES)
def test_identities_beyond_the_limit(size):
    """(2) Measured on an MI355X, in units of 2^-53 (the cpu backend's in brackets; at 16385 it is not run and the bound is one floor,
    64): DESIGN.md section 24 has the table."""
    n = bk.beyond_size(size)
    record_parity(f"toeplitz_levinson/identities/n{n}", **lv.check_identities_beyond("hip", n))


def test_independence():
    record_parity("toeplitz_levinson/independence", sld=lv.check_independence("hip", _beyond()))


def test_first_columns_in_two_launches():
    record_parity("toeplitz_levinson/chunk_loop", info=lv.check_chunk_loop("hip", _beyond()))


def test_failures():
    record_parity("toeplitz_levinson/failures", info=lv.check_failures("hip", _beyond()))


def test_other_routes_are_undisturbed_and_their_clocks_are_not_charged():
    record_parity("toeplitz_levinson/clocks", **lv.check_other_routes_undisturbed())


@pytest.mark.parametrize("name", [c[0] for c in gc.MODEL_CLASSES])
def test_model_layer(name):
    """(6) At n = 513 the batch with ``toeplitz_grad_method="blocked"`` equals the ``"columns"`` result bit for bit, and its values are
    those of ``toeplitz_method="blocked"``."""
    col, blk, vals = lv.check_model_gradient_equal("hip", name, 513)
    assert [v[0] for v in blk] == list(vals)
    assert lv._grads_equal(col, blk)
    record_parity(f"toeplitz_levinson/model/{name}_n513", lml=[float(v[0]) for v in blk])


def test_fit_predict_and_loo_beyond_the_limit():
    record_parity("toeplitz_levinson/fit_n8193", relative_difference=lv.check_fit_beyond_the_limit("hip"))


def test_the_pinned_refusals_still_raise():
    n = 8193
    t = tc.kms_column(n, 0.5)
    Z = np.ones((n, 1))
    for refused in (lambda: gm.toeplitz_grad(t, t[None], Z), lambda: gm.toeplitz_solve(t, Z), lambda: gm.toeplitz_inverse_column(t),
                    lambda: gm.toeplitz_inverse_diagonal(t), lambda: gm.toeplitz_loo(t, Z)):
        with pytest.raises(ValueError, match="n must be <= 8192"):
            refused()
    assert gm.toeplitz_inverse_column(t, method="blocked")[1] == 0
    X = np.linspace(0, 1, n)[:, None]
    y = np.random.RandomState(1).randn(n, 2)
    with pytest.raises(ValueError, match="n must be <= 8192"):
        lv.beyond_process("hip").fit(X, y, structure="toeplitz", dense_factor=False, toeplitz_method="blocked")
