"""The two kernels of gcc_pack_graphs keep no scratch on gfx950 (read off the code object's metadata, no GPU): a spill would put
a memory round trip into a kernel whose only job is moving bytes."""
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

SRC = isa_chains.ROOT / "gcc_amd" / "csrc" / "graph_batch.hip"


@pytest.fixture(scope="module")
def isa():
    return isa_chains.isa_of(SRC)


@pytest.mark.parametrize("kernel", ["pack_prefix_kernel", "pack_copy_kernelILi4E", "pack_copy_kernelILi2E"])
def test_pack_kernels_have_no_scratch(isa, kernel):
    md = _metadata(isa, kernel)
    assert md["private_segment_fixed_size"] == 0, md
    assert md.get("vgpr_spill_count", 0) == 0, md
