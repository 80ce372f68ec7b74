"""The fine-tuning head kernel and clip-by-value Adam keep no scratch on gfx950 (read off the code object's metadata, no GPU):
a spill in either would put a slow memory round trip inside every fine-tuning step."""
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

CSRC = isa_chains.ROOT / "gcc_amd" / "csrc"


@pytest.mark.parametrize("kernel", ["cls_head_kernelILb1E", "cls_head_kernelILb0E", "tail_value_kernelILi0E"])
def test_head_and_clipvalue_adam_have_no_scratch(kernel):
    md = _metadata(isa_chains.isa_of(CSRC / ("cls_head.hip" if kernel.startswith("cls_head") else "step_tail.hip")), kernel)
    assert md["private_segment_fixed_size"] == 0, md
    assert md.get("vgpr_spill_count", 0) == 0, md
