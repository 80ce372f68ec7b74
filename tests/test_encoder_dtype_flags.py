"""Host side of ``--encoder-dtype``: the flag, its default, the run name it must not change, and the encoder a checkpoint written
before the flag existed builds (generate.py and --finetune go through gcc_amd.encoder.encoder_from_opt)."""
import argparse
import copy

import pytest

import train
from gcc_amd.encoder import GraphEncoder, encoder_from_opt


def test_default_is_f32():
    assert train.parse_option([]).encoder_dtype == "f32"


def test_flag_parses_and_refuses_other_values():
    assert train.parse_option(["--encoder-dtype", "bf16"]).encoder_dtype == "bf16"
    assert train.parse_option(["--encoder-dtype", "f32"]).encoder_dtype == "f32"
    with pytest.raises(SystemExit):
        train.parse_option(["--encoder-dtype", "fp8"])


def test_model_name_does_not_carry_the_flag(tmp_path):
    base = ["--hidden-size", "128", "--model-path", str(tmp_path / "m"), "--tb-path", str(tmp_path / "t")]
    a = train.option_update(train.parse_option(base))
    b = train.option_update(train.parse_option(base + ["--encoder-dtype", "bf16", "--nce-dtype", "bf16"]))
    assert a.model_name == b.model_name and "bf16" not in b.model_name


def _opt(tmp_path, hidden, **kw):
    """the options a checkpoint of such a run stores (train.py:133-166 fills in the names)"""
    return train.option_update(train.parse_option(["--hidden-size", str(hidden), "--model-path", str(tmp_path / "m"), "--tb-path",
                                                   str(tmp_path / "t")] + sum(([f"--{k.replace('_', '-')}", str(v)] for k, v in kw.items()), [])))


def test_old_checkpoint_opt_builds_an_f32_encoder(tmp_path):
    opt = _opt(tmp_path, 128)
    old = argparse.Namespace(**{k: v for k, v in vars(copy.deepcopy(opt)).items() if k != "encoder_dtype"})
    assert not hasattr(old, "encoder_dtype")
    enc = encoder_from_opt(old)
    assert isinstance(enc, GraphEncoder) and enc.wide and enc.encoder_dtype == "f32"
    assert encoder_from_opt(opt).encoder_dtype == "f32"


def test_checkpoint_opt_with_the_flag_builds_a_bf16_encoder(tmp_path):
    enc = encoder_from_opt(_opt(tmp_path, 128, encoder_dtype="bf16"))
    assert enc.wide and enc.encoder_dtype == "bf16" and enc.hidden == enc.output_dim == 128
    with pytest.raises(NotImplementedError, match="compute in f32"):
        encoder_from_opt(_opt(tmp_path, 64, encoder_dtype="bf16"))


def test_engine_default_is_the_parity_entry_point():
    import inspect

    from gcc_amd.contrast import MemoryMoCo, WideNceEngine, e2e_logits

    assert inspect.signature(WideNceEngine.__init__).parameters["dtype"].default == "f32"
    assert inspect.signature(MemoryMoCo.__init__).parameters["nce_dtype"].default == "f32"
    assert inspect.signature(e2e_logits).parameters["nce_dtype"].default == "f32"
    assert inspect.signature(GraphEncoder.__init__).parameters["encoder_dtype"].default == "f32"
    assert list(inspect.signature(GraphEncoder.__init__).parameters)[-1] == "encoder_dtype"       # a trailing keyword
    assert MemoryMoCo(128, None, 96, 0.07, use_softmax=True, nce_dtype="bf16").wide
