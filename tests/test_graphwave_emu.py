"""The GraphWave kernels (gcc_amd/csrc/graphwave.hip) on the lock-step emulator against the reference's own runs and the NumPy
restatement: the checks of tests/graphwave_check.py on the fixtures of n <= 300 and d <= 64, plus n40d256."""
import numpy as np
import pytest

from tests import graphwave_check as C
from tests import graphwave_reference as R
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_logreg import emu_ptr


@pytest.fixture(scope="module")
def gw():
    return C.Gw(emu_lib(), emu_ptr, "cpu")


@pytest.mark.parametrize("name", R.EMU_FIXTURES)
def test_table_is_the_references(gw, name):
    C.check_parity(gw, name)


@pytest.mark.parametrize("name", ["n65d8", "n300d16"])
def test_heat_stage_zeroes_the_references_entries_and_keeps_the_rest(gw, name):
    C.check_heat(gw, name)


def test_heat_between_two_components_is_exactly_zero(gw):
    C.check_components(gw)


@pytest.mark.parametrize("name", ["n257d64", "hub300d8"])
def test_two_calls_and_a_panel_of_64_columns_give_the_same_bits(gw, name):
    C.check_bits(gw, name)


def test_uniform_multiplicity_cancels(gw):
    C.check_uniform_multiplicity(gw)


def test_broken_csr_sets_the_status_bit_and_writes_no_nan(gw):
    C.check_status_bits(gw)


def test_limits_short_workspace_and_null_members_are_refused_by_name(gw):
    C.check_refusals(gw)


def test_product_path_refuses_cpu_tensors():
    C.check_cpu_tensor_refused(emu_lib())


@pytest.mark.parametrize("name", R.FIXTURES)
def test_numpy_restatement_is_pinned_to_the_fixtures(name):
    fx = R.fixture(name)
    out = R.restatement(name)
    assert float(np.abs(out["chi"] - fx["chi"]).max()) <= R.VARIANT_FACTOR * fx["variant_distance"]
    assert not out["chi"][np.diff(fx["row_ptr"]) == 0].any()
    if "heat_print" in fx:
        assert np.array_equal(out["heat"] == 0, fx["heat_print"] == 0)


def test_the_threshold_bites_in_the_fixtures():
    """more than 5 % of the non-zero entries zeroed, some of them negative, in at least one fixture (the generating script's figures)"""
    assert any(float(R.fixture(n)["zeroed"]) > 0.05 and float(R.fixture(n)["zeroed_negative"]) > 0 for n in R.FIXTURES)


def test_coefficients_reproduce_the_heat_kernel():
    """sum_k c_k T_k(x) = exp(-tau (x + 1)) on [-1, 1], to the truncation of order 30"""
    x = np.linspace(-1, 1, 41)
    for tau in (0.3, 2.0, R.auto_taus(300)[1]):
        c = R.cheb_coefficients(tau)
        assert c.shape == (31,)
        assert float(np.abs(np.polynomial.chebyshev.chebval(x, c) - np.exp(-tau * (x + 1))).max()) <= 1e-12
    assert np.array_equal(R.time_points(4), [0.0]) and R.time_points(256).shape == (64,) and R.time_points(256)[-1] == 100.0
