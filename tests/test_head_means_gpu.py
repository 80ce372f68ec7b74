"""The four-launch MoCo head with its means in the ticket mode and deferred to the backward call, on the device:
tests/head_means_check.py's cases, both modes bit for bit against what the library of the commit before wrote on the device
(tests/golden/head_means_bits_gpu.npz)."""
import pytest

from tests import head_means_check as C
from tests import nce_check as N

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(C.cases()))
def test_head_means_case_on_the_device(name):
    C.check_case(N.head("gpu"), "gpu", name)


def test_more_than_64_slices_on_the_device():
    C.check_many_slices("gpu")


def test_deferred_forward_leaves_the_means_alone_on_the_device():
    C.deferred_forward_leaves_the_means_alone(N.head("gpu"))
