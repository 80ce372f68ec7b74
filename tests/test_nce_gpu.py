"""The MoCo / InfoNCE head, the enqueue, the EMA update, the gradient norm and Adam (gcc_amd/csrc/nce.hip, step_tail.hip) on a real MI355X:
every check of tests/test_nce_emu.py and tests/test_nce_onepass_emu.py (tests/nce_check.py) at the smallest shapes that still
reach each path -- a last slice shorter than a chunk, a last slice of one row, B = 63 / 65, more than 64 slices, patch rows
that wrap, several query blocks of the E2E head.

Why a device tier: the reason tests/test_train_step_gpu.py::test_fused_step_reproduces_reference_post_step_state gives.  The
emulator executes workgroups one after another and cannot see ordering / visibility bugs; this can.  Here that is the
reduction by the workgroup that arrives last (a ticket atomic, a device-wide fence and cache-bypassing loads in
nce_mean_by_last, nce_combine_kernel and gradnorm_kernel), the operand layouts of the real matrix instructions, the device's
expf / logf, and loads requested ahead of a __syncthreads."""
import pytest

from tests import nce_check as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    return C.head("gpu")


# ------------------------------------------------------------------------------------------- tests/test_nce_emu.py's checks
def test_moco_head_matches_reference_golden(S):
    C.check_moco_golden(S)


@pytest.mark.parametrize("B,K", C.RAGGED)
def test_moco_head_ragged_shapes_vs_oracle(S, B, K):
    C.check_ragged_vs_oracle(S, B, K)


def test_e2e_head_matches_reference_golden(S):
    C.check_e2e_golden(S)


def test_ema_matches_moment_update(S):
    C.check_ema(S)


@pytest.mark.parametrize("B,K", [(6, 48), (70, 200)])
def test_bf16_head_equals_the_oracle_on_rounded_operands_and_bounds_the_distance_to_f32(S, B, K):
    C.check_bf16_head(S, B, K)


# ----------------------------------------------------------------------------------- tests/test_nce_onepass_emu.py's checks
@pytest.mark.parametrize("K", C.ONEPASS_K)
@pytest.mark.parametrize("B", C.ONEPASS_B)
def test_onepass_head_shapes(S, B, K):
    C.check_onepass_shape(S, B, K)


def test_more_than_64_slices_by_workgroup_count():
    C.check_more_than_64_slices("gpu")


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


# ------------------------------------------------------------------------------------------------------- the newer cases
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", C.E2E_B)
def test_e2e_head_ragged_batch_sizes(S, B, dtype):
    C.check_e2e_ragged(S, B, dtype)


@pytest.mark.parametrize("B,K", C.BIT_SHAPES)
def test_identical_calls_give_identical_bits(S, B, K):
    C.check_identical_calls_give_identical_bits(S, B, K)


def test_interleaved_one_pass_and_four_launch_calls_share_a_workspace(S):
    C.check_interleaved_calls_on_one_engine(S)


def test_side_stream_gives_the_default_streams_bits(S):
    C.check_side_stream_gives_the_default_streams_bits(S)


@pytest.mark.parametrize("n", C.ADAM_N)
def test_adam_step_ragged_sizes(S, n):
    C.check_adam(S, n)


@pytest.mark.parametrize("tail", C.ADAM_TAILS)
@pytest.mark.parametrize("n", C.ADAM_N)
def test_adam_ema_step_ragged_sizes_and_tail_past_the_live_prefix(S, n, tail):
    C.check_adam(S, n, tail)


@pytest.mark.parametrize("n", C.ADAM_N)
def test_ema_ragged_sizes(S, n):
    C.check_ema_ragged(S, n)


def test_enqueue_full_queue_wrap_at_the_first_key_and_refusal(S):
    C.check_enqueue(S)
