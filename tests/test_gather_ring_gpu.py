"""The ring of row requests in the neighbour gather on the device: tests/gather_ring_check.py's cases against float64 sums and,
bit for bit, against what the library of the commit before the ring wrote on the device
(tests/golden/gather_ring_bits_gpu.npz)."""
import pytest

from tests import gather_ring_check as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(K.cases()))
def test_gather_ring_case_on_the_device(name):
    K.check_case(K.Tier("gpu"), name)
