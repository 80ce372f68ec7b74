"""The ring of row requests in the neighbour gather on the wave64 emulator: tests/gather_ring_check.py's cases against float64
sums and, bit for bit, against what the library of the commit before the ring wrote on this tier
(tests/golden/gather_ring_bits_emu.npz)."""
import pytest

from tests import gather_ring_check as K


def test_the_cases_cross_the_boundaries_they_are_named_for():
    K.check_cases_cross_their_boundaries()


@pytest.mark.parametrize("name", list(K.cases()))
def test_gather_ring_case_on_the_emulator(name):
    K.check_case(K.Tier("emu"), name)
