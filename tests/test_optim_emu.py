"""The Adam / SGD / Adagrad tails (gcc_adam_*_step, gcc_opt_step, gcc_opt_ema_step[_scalars], gcc_opt_clipvalue_step of
gcc_amd/csrc/step_tail.hip) on the
wave64 emulator build: every check of tests/optim_check.py against torch.optim on CPU float32."""
import pytest

from tests import optim_check as C

@pytest.fixture(scope="module")
def S():
    return C.head("emu")


@pytest.mark.parametrize("tail", [None] + C.ADAM_TAILS)
@pytest.mark.parametrize("n", C.ADAM_N)
@pytest.mark.parametrize("rule", C.ALL_RULES)
def test_clip_by_norm_tail_matches_torch_at_ragged_sizes(S, rule, n, tail):
    C.check_norm_sizes(S, rule, n, tail)


@pytest.mark.parametrize("rule,var,wd,max_norm,grad_scale", C.NORM_GRID)
def test_clip_by_norm_tail_matches_torch_over_the_rule_variations(S, rule, var, wd, max_norm, grad_scale):
    C.check_norm_grid(S, rule, var, wd, max_norm, grad_scale)


@pytest.mark.parametrize("n", C.ADAM_N)
@pytest.mark.parametrize("rule", C.ALL_RULES)
def test_clip_by_value_tail_matches_torch_at_ragged_sizes(S, rule, n):
    C.check_value_sizes(S, rule, n)


@pytest.mark.parametrize("tail", [None, 37])
@pytest.mark.parametrize("n", C.CAP_N)
@pytest.mark.parametrize("rule", C.ALL_RULES)
def test_clip_by_norm_tail_matches_torch_around_the_workgroup_cap(S, rule, n, tail):
    C.check_norm_sizes(S, rule, n, tail)


@pytest.mark.parametrize("n", C.CAP_N)
@pytest.mark.parametrize("rule", C.ALL_RULES)
def test_clip_by_value_tail_matches_torch_around_the_workgroup_cap(S, rule, n):
    C.check_value_sizes(S, rule, n)


@pytest.mark.parametrize("nparts", C.FOLD_NPARTS)
def test_adam_with_the_sum_of_squares_as_partials_equals_the_separate_launch(S, nparts):
    C.check_folded_partials(S, nparts)


@pytest.mark.parametrize("rule,var,wd,clip,grad_scale", C.VALUE_GRID)
def test_clip_by_value_tail_matches_torch_over_the_rule_variations(S, rule, var, wd, clip, grad_scale):
    C.check_value_grid(S, rule, var, wd, clip, grad_scale)


def test_adagrad_zero_gradient_on_zero_state_keeps_the_parameters(S):
    C.check_adagrad_zero_gradient(S)


@pytest.mark.parametrize("rule", C.ALL_RULES)
def test_device_scalars_give_the_by_value_bits(S, rule):
    C.check_scalars_give_the_by_value_bits(S, rule)


@pytest.mark.parametrize("rule", C.ALL_RULES)
def test_identical_calls_give_identical_bits(S, rule):
    C.check_identical_calls_give_identical_bits(S, rule)


@pytest.mark.parametrize("rule", C.ALL_RULES)
def test_ema_step_without_ema_and_meters_is_opt_step(S, rule):
    C.check_ema_step_without_extras_is_opt_step(S, rule)


def test_unknown_rule_empty_buffer_and_null_state_are_refused_by_name(S):
    C.check_refusals(S)
