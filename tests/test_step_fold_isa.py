"""The kernels the folded MoCo step added to or changed keep no scratch on gfx950, and the two new head kernels have no
load-wait ladders (read off the code object's metadata and the ISA listing, no GPU)."""
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

CSRC = isa_chains.ROOT / "gcc_amd" / "csrc"


@pytest.mark.parametrize("src,kernel", [("nce.hip", "nce_onepass_kernel"), ("nce.hip", "nce_merge_kernel"), ("step_tail.hip", "tail_norm_kernelILi0E"),
                                        ("encoder_bwd.hip", "gin_grad_final_kernel"), ("encoder.hip", "gin_feat_kernel")])
def test_no_scratch(src, kernel):
    md = _metadata(isa_chains.isa_of(CSRC / src), kernel)
    assert md["private_segment_fixed_size"] == 0, md
    assert md.get("vgpr_spill_count", 0) == 0, md


def test_new_head_kernels_have_no_load_wait_ladders():
    text = isa_chains.isa_of(CSRC / "nce.hip")
    seen = set()
    for name, body in isa_chains.kernels(text):
        m = re.search(r"\d+(nce_(?:onepass|merge)_kernel)", name)
        if m:
            seen.add(m.group(1))
            chain = isa_chains.chain(body)
            assert "LWLWLWLW" not in chain, (m.group(1), chain)
    assert seen == {"nce_onepass_kernel", "nce_merge_kernel"}
