"""The one-pass MoCo head (gcc_nce_forward_backward: nce_onepass_kernel + nce_merge_kernel of gcc_amd/csrc/nce.hip) on the
wave64 emulator against the four-launch head (gcc_nce_forward + gcc_nce_backward) and against a float64 restatement in
torch: loss, prob, lse, pos, dq; and the fixed-order claims of nce.hip (identical bits from identical calls, calls of two
shapes interleaved on one engine).  The checks and their tolerances are tests/nce_check.py's, which tests/test_nce_gpu.py
runs on the device."""
import pytest

from tests import nce_check as C


@pytest.fixture(scope="module")
def S():
    return C.head("emu")


# K = 100: two slices, the last one 36 rows (shorter than a 64-row chunk); K = 4097: the last slice is ONE row (B <= 64: 65
# slices of 64 rows -- past the merge kernel's first 64 --, B = 65: 128-row slices, B = 256: 33 slices of 128); K = 200 at
# B > 64: slices of 64 rows with a last one of 8
@pytest.mark.parametrize("K", C.ONEPASS_K)
@pytest.mark.parametrize("B", C.ONEPASS_B)
def test_onepass_head_shapes(S, B, K):
    C.check_onepass_shape(S, B, K)


def test_more_than_64_slices_by_workgroup_count():
    C.check_more_than_64_slices("emu")


@pytest.mark.parametrize("B,K", [(5, 300), (70, 1000)])
def test_logits_reach_plus_minus_60(S, B, K):
    C.check_logits_reach_plus_minus_60(S, B, K)


@pytest.mark.parametrize("order", ["increasing", "decreasing"])
def test_monotonic_maximum_along_the_queue(S, order):
    C.check_monotonic_maximum(S, order)


def test_lane_groups_of_a_query_need_one_common_maximum(S):
    C.check_lane_groups(S)


def test_patch_rows_and_dloss(S):
    C.check_patch_rows_and_dloss(S)


def test_bf16_keeps_the_four_launches(S):
    C.check_bf16_keeps_the_four_launches(S)


@pytest.mark.parametrize("B,K", C.BIT_SHAPES)
def test_identical_calls_give_identical_bits(S, B, K):
    C.check_identical_calls_give_identical_bits(S, B, K)


def test_interleaved_one_pass_and_four_launch_calls_share_a_workspace(S):
    C.check_interleaved_calls_on_one_engine(S)
