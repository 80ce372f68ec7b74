"""The SGD / Adagrad tails keep no scratch on gfx950 (read off the code object's metadata, no GPU): a spill would put a slow memory
round trip inside every training step's last launch."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_chains  # noqa: E402
from tests.test_solver_footprint import _metadata  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(isa_chains.HIPCC) or shutil.which("make") is None,
                                reason="hipcc not installed")

SRC = isa_chains.ROOT / "gcc_amd" / "csrc" / "step_tail.hip"


@pytest.mark.parametrize("kernel", ["tail_norm_kernelILi1E", "tail_norm_kernelILi2E", "tail_value_kernelILi1E", "tail_value_kernelILi2E"])
def test_sgd_and_adagrad_tails_have_no_scratch(kernel):
    md = _metadata(isa_chains.isa_of(SRC), kernel)
    assert md["private_segment_fixed_size"] == 0, md
    assert md.get("vgpr_spill_count", 0) == 0, md
