"""The GraphWave kernels (gcc_amd/csrc/graphwave.hip) on a real MI355X against the reference's own runs and the NumPy
restatement: the checks of tests/graphwave_check.py on every fixture."""
import pytest

from tests import graphwave_check as C
from tests import graphwave_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gw():
    from gcc_amd import _cabi

    return C.Gw(_cabi.load(), _cabi.dev_ptr, "cuda:0")


@pytest.mark.parametrize("name", R.FIXTURES)
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


def test_cpu_tensor_is_refused(gw):
    C.check_cpu_tensor_refused(gw.lib)
