"""The sparse block class's matrix build, Cholesky and expansion on the device: the cases of
tests/posemb_block_build_cases.py against the strict invariants and, bit for bit, against what the library of the commit
before wrote on the device (tests/golden/posemb_block_build_bits_gpu.npz)."""
import pytest

from tests import test_posemb_emu as T
from tests.test_posemb_block_build_emu import CASES, check_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_block_build_case_on_device(name, monkeypatch):
    check_case("gpu", name, T._check, lambda h: monkeypatch.setattr(T, "HID", h))
