"""The backward tail's degree-embedding gradient on the wave64 emulator: tests/bwd_tail_check.py's cases against the fixed tree over the
partial tables, float64 sums and, bit for bit, the recording of this tier (tests/golden/bwd_tail_bits_emu.npz)."""
import pytest

from tests import bwd_tail_check as C
from tests import gather_ring_check as K


def test_the_cases_are_what_they_are_named_for():
    C.check_cases_are_what_they_are_named_for()


@pytest.mark.parametrize("name", list(C.cases()))
def test_bwd_tail_case_on_the_emulator(name):
    C.check_case(K.Tier("emu"), name)
