"""The grid search over C (gcc_svc_search_*, gcc_amd/csrc/svc.hip) on the lock-step emulator: the checks of
tests/svc_search_check.py.  Every case stays below the 10^5 SMO iterations that tests/test_svc_emu.py runs (the golden corpus:
about 30,000, recorded by make_graphcls_search_golden.py) except the four-wave case -- 2,400 rows, inner problems of 600 -- which
runs on the GPU only."""
import pytest

from tests import svc_search_check as C
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_svc import emu_ptr


@pytest.fixture(scope="module")
def svc():
    return C.Svc(emu_lib(), emu_ptr, "cpu")


def test_search_is_bit_equal_to_the_composition_of_plain_fits(svc):
    C.check_equals_composition(svc, "small")


def test_launch_split_is_bit_equal_to_one_launch(svc):
    C.check_launch_split(svc)


def test_ties_go_to_the_earlier_candidate_and_the_mean_is_numpys(svc):
    C.check_ties_and_mean(svc)


def test_reference_shape_agrees_with_sklearn_grid_search(svc):
    C.check_against_sklearn(svc)


def test_inner_missing_class_is_reported_apart_and_does_not_fail(svc):
    C.check_inner_missing_class(svc)


def test_single_class_inner_side_is_refused_before_any_launch(svc, monkeypatch):
    C.check_single_class_inner_side(svc, monkeypatch)


def test_limits_are_refused_by_name(svc):
    C.check_limits(svc)


def test_status_bits_on_the_search_path(svc):
    C.check_status_bits(svc)


def test_iteration_cap_of_an_inner_problem_only_warns(svc):
    C.check_iteration_cap_only_warns(svc)


def test_short_workspace_sets_overflow_and_stays_inside(svc, monkeypatch):
    C.check_short_workspace(svc, monkeypatch)
