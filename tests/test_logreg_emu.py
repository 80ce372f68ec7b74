"""The logistic-regression kernels (gcc_amd/csrc/logreg.hip) on the lock-step emulator against sklearn's converged fits: the
checks of tests/logreg_check.py on the fixtures of N <= 300 and D <= 17.  Wider shapes run on the GPU only."""
import pytest

from tests import logreg_check as C
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_logreg import emu_ptr


@pytest.fixture(scope="module")
def lr():
    return C.Lr(emu_lib(), emu_ptr, "cpu")


@pytest.mark.parametrize("name", C.EMU_FIXTURES)
def test_fit_is_the_minimiser_sklearn_converges_to(lr, name):
    C.check_fit(lr, name)


@pytest.mark.parametrize("name", C.PENALISED)
def test_penalised_intercept_agrees_with_liblinear(lr, name):
    C.check_fit(lr, name, rho=1.0)


def test_sync_split_is_bit_equal_binary(lr):
    fx = C.fixture("a")
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


def test_product_path_refuses_cpu_tensors():
    C.check_cpu_tensor_refused(emu_lib())
