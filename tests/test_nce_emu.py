"""Kernel-logic parity on CPU for the MoCo / InfoNCE head (gcc_amd/csrc/nce.hip on the wave64 emulator) vs the
reference-generated golden vectors and the oracle, and for the E2E head at ragged batch sizes, the optimizer tail at ragged
sizes and the enqueue against float64 restatements: the checks of tests/nce_check.py, which tests/test_nce_gpu.py runs on the
device."""
import pytest

from gcc_amd.contrast import NceEngine
from tests import nce_check as C
from tests.hipemu.emu_driver import emu_lib


def emu_nce():
    return NceEngine(lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr())


@pytest.fixture(scope="module")
def S():
    return C.head("emu")


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


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", C.E2E_B)
def test_e2e_head_ragged_batch_sizes(S, B, dtype):
    C.check_e2e_ragged(S, B, dtype)


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
