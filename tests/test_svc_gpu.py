"""The C-SVC kernels (gcc_amd/csrc/svc.hip) on a real MI355X against sklearn's SVC: the checks of tests/svc_check.py.
Fixture (e) -- about 80,000 iterations -- runs here only."""
import pytest

from tests import svc_check as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def svc():
    from gcc_amd import _cabi

    return C.Svc(_cabi.load(), _cabi.dev_ptr, "cuda:0")


@pytest.mark.parametrize("N,D,extra", C.DISTANCE_SHAPES)
def test_distances_bit_symmetric_zero_diagonal_and_close_to_float64(svc, N, D, extra):
    C.check_distances(svc, N, D, extra)


def test_non_finite_embeddings_set_their_status_bit(svc):
    C.check_nonfinite(svc)


@pytest.mark.parametrize("name", ["a", "b", "c", "e"])
def test_binary_fit_agrees_with_sklearn(svc, name):
    C.check_binary(svc, name)


def test_binary_fit_over_several_launches_agrees_with_sklearn(svc):
    res = C.check_binary(svc, "d", iters_per_launch=4096)
    assert res["launches"] >= 3


@pytest.mark.parametrize("name", ["a", "c"])
def test_launch_split_is_bit_equal_to_one_launch(svc, name):
    C.check_launch_split(svc, name)


def test_iteration_cap_is_reported(svc):
    C.check_iteration_cap(svc)


@pytest.mark.parametrize("name", ["m3", "m5"])
def test_multiclass_votes_agree_with_sklearn(svc, name):
    C.check_multiclass(svc, name)


def test_three_way_vote_tie_goes_to_the_lowest_class(svc):
    C.check_vote_tie(svc)


def test_single_row_class_and_two_row_problem(svc):
    C.check_single_row_class_and_two_row_problem(svc)


def test_all_alpha_at_the_bound(svc):
    C.check_all_alpha_at_bound(svc)


def test_problem_size_limit_is_refused_by_name(svc):
    C.check_problem_size_limit(svc)


def test_each_status_bit(svc, monkeypatch):
    C.check_status_bits(svc, monkeypatch)


def test_many_rows_take_the_four_wave_kernel(svc):
    C.check_four_wave_kernel(svc)


def test_launch_split_with_more_than_64_kib_of_lds(svc):
    C.check_large_lds_launch_split(svc)
