"""The fused steps with --optimizer sgd / adagrad on a real MI355X: the checks of tests/test_optim_step_emu.py
(tests/optim_step_check.py) with the gfx950 library, and -- what only a device can run -- hipGraph replay of the step against the
launch-by-launch step, bit for bit."""
import pytest

from tests import optim_step_check as C

pytestmark = pytest.mark.gpu
TIER = C.GPU

RULES = ["sgd", "adagrad"]


@pytest.mark.parametrize("rule", RULES)
def test_fused_moco_step_matches_the_api_composition(rule):
    C.check_moco(TIER, rule)


def test_wide_moco_step_with_sgd_takes_the_by_value_route():
    C.check_moco(TIER, "sgd", wide=True)


@pytest.mark.parametrize("rule", RULES)
def test_fused_e2e_step_matches_the_api_composition(rule):
    C.check_e2e(TIER, rule)


@pytest.mark.parametrize("rule", RULES)
def test_fused_finetune_step_matches_the_api_composition(rule):
    C.check_finetune(TIER, rule)


@pytest.mark.parametrize("rule", RULES)
def test_state_dict_round_trip_and_the_callers_learning_rate(rule):
    C.check_state_dict_and_param_group_lr(TIER, rule)


@pytest.mark.parametrize("rule", RULES)
def test_graph_replay_ends_with_the_eager_steps_bits(rule):
    C.check_graph_replay_gives_the_eager_bits(rule)
