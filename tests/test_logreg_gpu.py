"""The logistic-regression kernels (gcc_amd/csrc/logreg.hip) on a real MI355X against sklearn's converged fits: the checks of
tests/logreg_check.py, with the wide fixtures (n < D, D = 64, and D = 129 / 256 where the Cholesky leaves LDS) that the emulator
tier leaves out."""
import pytest

from tests import logreg_check as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lr():
    from gcc_amd import _cabi

    return C.Lr(_cabi.load(), _cabi.dev_ptr, "cuda:0")


@pytest.mark.parametrize("name", C.GPU_FIXTURES)
def test_fit_is_the_minimiser_sklearn_converges_to(lr, name):
    C.check_fit(lr, name)


@pytest.mark.parametrize("name", C.PENALISED + ["w64"])
def test_penalised_intercept_agrees_with_liblinear(lr, name):
    C.check_fit(lr, name, rho=1.0)


@pytest.mark.parametrize("name", ["a", "c129"])
def test_sync_split_is_bit_equal_binary(lr, name):
    fx = C.fixture(name)
    C.check_sync_split(lr, lambda **kw: lr.fit(fx["X"], fx["y"], fx["fold"], **kw))


def test_sync_split_is_bit_equal_many_problems(lr):
    X, y, fold = C.rule_fixture()
    C.check_sync_split(lr, lambda **kw: lr.fit(X, y, fold, **kw))


def test_top_k_ties_empty_rows_and_constant_columns(lr):
    C.check_rules(lr)


def test_multilabel_ten_folds_agree_with_sklearn(lr):
    C.check_multilabel(lr)


def test_each_status_bit(lr):
    C.check_status_bits(lr)


def test_limits_short_workspace_and_null_members_are_refused_by_name(lr):
    C.check_refusals(lr)


def test_cpu_tensor_is_refused(lr):
    C.check_cpu_tensor_refused(lr.lib)
