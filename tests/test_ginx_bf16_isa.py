"""ginx_gemm_bf16_kernel on gfx950, read off the ISA listing and the code object's metadata (no GPU): its products run on the bf16
matrix instruction and on nothing else, its operands come out of LDS 16 bytes per lane, it keeps no scratch -- and the f32 kernel
next to it compiles to exactly the listing it had before the bf16 kernel was added."""
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

F32_KERNEL_INSTRUCTIONS = 1223      # ginx_gemm_kernel before this kernel existed (hipcc -O3 --offload-arch=gfx950)


@pytest.fixture(scope="module")
def listing():
    return isa_chains.isa_of(isa_chains.ROOT / "gcc_amd" / "csrc" / "ginx.hip")


def _ops(text, kernel):
    """mnemonics of the one kernel whose mangled name ends in <len><kernel>ENS_8GemmArgsE"""
    found = [body for name, body in isa_chains.kernels(text) if re.search(rf"\d+{kernel}E", name)]
    assert len(found) == 1, kernel
    return [s.split()[0] for s in found[0] if s and not s.startswith((";", ".")) and not s.endswith(":")]


def test_bf16_kernel_uses_the_bf16_matrix_instruction_only(listing):
    ops = _ops(listing, "ginx_gemm_bf16_kernel")
    mfma = [o for o in ops if o.startswith("v_mfma")]
    assert mfma and all(o in ("v_mfma_f32_16x16x32_bf16", "v_mfma_f32_32x32x16_bf16") for o in mfma), sorted(set(mfma))
    assert "v_mfma_f32_16x16x4_f32" not in ops
    # two k-steps of 32 x (2 x 2 fragments) per 64-wide k-tile, in one loop body
    assert len(mfma) == 8, len(mfma)


def test_bf16_kernel_reads_its_operands_16_bytes_per_lane(listing):
    ops = _ops(listing, "ginx_gemm_bf16_kernel")
    wide = [o for o in ops if o in ("ds_read_b128", "ds_load_b128")]
    assert len(wide) == 8, len(wide)                        # 2 A + 2 B fragments per k-step
    # no narrower LDS read feeds the products: every ds_read of the kernel is one of those
    assert [o for o in ops if o.startswith(("ds_read", "ds_load"))] == wide
    # the staging writes whole 8-value rows, converted two at a time
    assert "ds_write_b128" in ops or "ds_store_b128" in ops
    assert "v_cvt_pk_bf16_f32" in ops


def test_bf16_kernel_keeps_no_scratch(listing):
    ops = _ops(listing, "ginx_gemm_bf16_kernel")
    assert not [o for o in ops if o.startswith("scratch_")]
    md = _metadata(listing, "ginx_gemm_bf16_kernel")
    assert md["private_segment_fixed_size"] == 0, md
    assert md.get("vgpr_spill_count", 0) == 0 and md.get("sgpr_spill_count", 0) == 0, md
    assert md["vgpr_count"] <= 128, md                      # four waves per SIMD
    assert md["group_segment_fixed_size"] == 2 * 64 * 144, md


def test_f32_kernel_is_unchanged(listing):
    ops = _ops(listing, "ginx_gemm_kernel")
    assert len(ops) == F32_KERNEL_INSTRUCTIONS, len(ops)
    assert "v_mfma_f32_16x16x4_f32" in ops and not [o for o in ops if "bf16" in o]
