"""The fine-tuning head and clip-by-value Adam (csrc/cls_head.hip, csrc/step_tail.hip) at their shape edges on the emulator build, against float64
torch.  The cases, inputs and bars are tests/cls_head_check.py's; the device tier is tests/test_cls_head_edges_gpu.py."""
import pytest

from tests import cls_head_check as H
from tests.wide_edges_check import EMU


@pytest.mark.parametrize("pattern", H.PATTERNS)
@pytest.mark.parametrize("B,C,D", H.SHAPES)
def test_head_shape_edges_vs_float64(B, C, D, pattern):
    H.check_shape(EMU, B, C, D, pattern)


def test_head_logits_that_need_the_max_subtraction():
    H.check_wide_logits(EMU)


def test_head_tie_goes_to_the_lower_class_in_a_later_row_of_a_group():
    H.check_ties(EMU)


def test_head_label_out_of_range_gives_nan_loss_and_finite_dlogits():
    H.check_label_out_of_range(EMU)


def test_head_eval_accumulates_and_repeats_the_train_logits():
    H.check_eval(EMU)


def test_head_autograd_wrapper_scales_the_gradients():
    H.check_autograd(EMU)


def test_head_two_runs_are_bit_identical():
    H.check_repeatable(EMU)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 131072, 131073, 300001])
def test_adam_clipvalue_sizes_vs_torch_adam(n):
    H.check_adam_clipvalue(EMU, n)
