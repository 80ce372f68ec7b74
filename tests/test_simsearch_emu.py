"""gcc_sim_search (gcc_amd/csrc/simsearch.hip) on the lock-step emulator against the float64 restatement of
tests/simsearch_check.py: every case in the exact tier (bit for bit) and in the normalised tier (within DELTA, every query),
the duplicate-row tie rule, the status bits, the refusals and the Python surface."""
import pytest

from tests import simsearch_check as C
from tests.hipemu.emu_driver import emu_lib


@pytest.fixture(scope="module")
def sim():
    return C.Sim(emu_lib(), lambda t: t.data_ptr() if t is not None else None, "cpu")


@pytest.mark.parametrize("tier", ["exact", "norm"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_search_equals_the_restatement(sim, name, tier):
    C.check_case(sim, name, tier)


def test_duplicate_rows_tie_bitwise_and_list_in_column_order(sim):
    C.check_duplicate_rows(sim)


def test_zero_row_sets_its_status_bit_and_scores_zero(sim):
    C.check_zero_row(sim)


def test_out_of_range_index_is_absent_with_a_status_bit(sim):
    C.check_bad_index(sim)


def test_bad_arguments_are_refused_by_name_with_nothing_written(sim):
    C.check_refusals(sim)


def test_engine_recall_and_argument_errors(sim):
    C.check_engine(sim)
