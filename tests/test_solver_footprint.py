"""Register and scratch footprint of the block eigensolver class (`posemb_cheb_kernel`), read off the gfx950 code
object's metadata (no GPU needed).

Scratch is where an item's time went: the parent of this test's change kept 964 bytes per lane in scratch (300 VGPRs
spilled), mostly thread-index arithmetic the compiler had hoisted out of the item loop.  The kernel makes the thread
index opaque per item, per round and per sparse product; these checks fail when that regresses.
The 512-thread instantiation is the starting point for sharing a CU with the training stream: it must keep compiling
under its register cap."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_chains  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(isa_chains.HIPCC) or shutil.which("make") is None,
                                reason="hipcc not installed")

SRC = isa_chains.ROOT / "gcc_amd" / "csrc" / "posemb.hip"


def _metadata(text, kernel):
    """the scalar fields of `kernel`'s entry in the amdhsa.kernels metadata of an assembly listing"""
    meta = text.split("amdhsa.kernels:", 1)[1]
    for entry in re.split(r"\n\s*- \.", meta):
        fields = dict(re.findall(r"\.?([a-z_]+):\s+(\S+)", "." + entry))
        if kernel in fields.get("name", ""):
            return {k: int(v) if re.fullmatch(r"-?\d+", v) else v for k, v in fields.items()}
    raise AssertionError(f"{kernel} not in the listing")


def test_default_block_class_keeps_its_scratch_small():
    md = _metadata(isa_chains.isa_of(SRC), "posemb_cheb_kernel")
    assert md["max_flat_workgroup_size"] == 1024
    assert md["vgpr_count"] <= 128
    assert md["private_segment_fixed_size"] <= 256, md
    assert md["vgpr_spill_count"] <= 128, md


def test_512_thread_block_class_compiles_under_its_register_cap():
    md = _metadata(isa_chains.isa_of(SRC, extra=("-DGCC_POSEMB_CH_THREADS=512",)), "posemb_cheb_kernel")
    assert md["max_flat_workgroup_size"] == 512
    assert md["vgpr_count"] + md.get("agpr_count", 0) <= 168, md      # two waves per SIMD leave one 168-VGPR wave free
    assert md["private_segment_fixed_size"] <= 128, md
