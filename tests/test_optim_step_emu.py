"""The fused steps with --optimizer sgd / adagrad on the wave64 emulator build (tests/optim_step_check.py): MoCoTrainStep at both
widths, E2ETrainStep and FinetuneTrainStep against autograd + torch's clip + torch.optim over the same kernels."""
import pytest

from tests import optim_step_check as C

TIER = C.EMU

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
