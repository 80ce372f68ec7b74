"""The fine-tuning head and clip-by-value Adam (csrc/cls_head.hip, csrc/step_tail.hip) at their shape edges on a real MI355X, against float64
torch.  The cases, inputs and bars are tests/cls_head_check.py's; the emulator tier is tests/test_cls_head_edges_emu.py.

Measured on an MI355X (worst error of loss, logits, dW, db, dfeat and dlogits against float64, as a share of the tensor's largest
entry): at most 1.1e-6 over the 33 shape x pattern cases (the largest at B 1025, C 21, D 100), 2.4e-6 with logits spread over 169;
clip-by-value Adam: at most 9.6e-7 absolute on a parameter after four steps (n = 300,001).  All 46 cases passed on first contact
with the device.  Wall time of the file: 4.5 s (1.4 s of it the first optimizer case, 0.2 s the first head case)."""
import pytest

from tests import cls_head_check as H
from tests.wide_edges_check import GPU

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pattern", H.PATTERNS)
@pytest.mark.parametrize("B,C,D", H.SHAPES)
def test_head_shape_edges_vs_float64_on_device(B, C, D, pattern):
    H.check_shape(GPU, B, C, D, pattern)


def test_head_logits_that_need_the_max_subtraction_on_device():
    H.check_wide_logits(GPU)


def test_head_tie_goes_to_the_lower_class_in_a_later_row_of_a_group_on_device():
    H.check_ties(GPU)


def test_head_label_out_of_range_gives_nan_loss_and_finite_dlogits_on_device():
    H.check_label_out_of_range(GPU)


def test_head_eval_accumulates_and_repeats_the_train_logits_on_device():
    H.check_eval(GPU)


def test_head_autograd_wrapper_scales_the_gradients_on_device():
    H.check_autograd(GPU)


def test_head_two_runs_are_bit_identical_on_device():
    H.check_repeatable(GPU)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 131072, 131073, 300001])
def test_adam_clipvalue_sizes_vs_torch_adam_on_device(n):
    H.check_adam_clipvalue(GPU, n)
