"""Every kernel of gcc_amd/csrc/text_ingest.hip keeps no scratch on gfx950 (read off the code object's metadata, no GPU): the reader
streams bytes once or twice, and a spill would put a memory round trip into every lane's sixteen of them."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_chains  # noqa: E402
from tests.test_solver_footprint import _metadata  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(isa_chains.HIPCC) or shutil.which("make") is None,
                                reason="hipcc not installed")

SRC = isa_chains.ROOT / "gcc_amd" / "csrc" / "text_ingest.hip"
KERNELS = sorted(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", SRC.read_text()))


@pytest.fixture(scope="module")
def isa():
    return isa_chains.isa_of(SRC)


def test_the_file_holds_the_kernels_its_header_lists():
    assert KERNELS == sorted(["ti_count_kernel", "ti_scan_kernel", "ti_parse_kernel", "ti_select_kernel"])
    header = SRC.read_text().split("#include")[0]
    for kernel in KERNELS:
        assert kernel in header, kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_has_no_scratch_and_no_spill(isa, kernel):
    md = _metadata(isa, kernel)
    assert md["private_segment_fixed_size"] == 0, md
    assert md.get("vgpr_spill_count", 0) == 0 and md.get("sgpr_spill_count", 0) == 0, md
