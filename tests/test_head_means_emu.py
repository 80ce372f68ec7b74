"""The four-launch MoCo head with its means in the ticket mode and deferred to the backward call, on the wave64 emulator:
tests/head_means_check.py's cases, both modes bit for bit against what the library of the commit before wrote on this tier
(tests/golden/head_means_bits_emu.npz)."""
import pytest

from tests import head_means_check as C
from tests import nce_check as N


def test_the_cases_are_what_they_are_named_for():
    C.check_cases_are_what_they_are_named_for()


@pytest.mark.parametrize("name", list(C.cases()))
def test_head_means_case_on_the_emulator(name):
    C.check_case(N.head("emu"), "emu", name)


def test_more_than_64_slices_on_the_emulator():
    C.check_many_slices("emu")


def test_deferred_forward_leaves_the_means_alone_on_the_emulator():
    C.deferred_forward_leaves_the_means_alone(N.head("emu"))
