"""The ORDER of the C-ABI calls of a training step, pinned against tests/golden/step_call_sequences.json: every trainer
(MoCoTrainStep at both widths, with and without device-resident scalars, the folded tail, the one-pass head, collectives at
world size 1; E2ETrainStep; FinetuneTrainStep) runs two steps on the emulator build with each engine's library behind a proxy
that logs the name of every ``gcc_*`` symbol it hands out.  The collectives cases also log where the key all-gather begins,
the gradient all-reduce runs and the all-gather is joined.  The fixture was recorded by this file before the host layer's step
bodies were merged into one; the numerics of the same steps are the other emulator tests' business."""
import json
import os

import pytest
import torch

from gcc_amd.contrast import MemoryMoCo
from gcc_amd.train_step import E2ETrainStep, MoCoTrainStep
from tests.hipemu.emu_encoder import emu_engine, reference_encoder
from tests.test_nce_emu import emu_nce
from tests.test_step_tail_emu import _sampler, _trainer
from tests.test_wide_edges_emu import _fused_step, _masks, _ScriptedSampler, encoder
from tests.test_wide_encoder_emu import emu_wide_engine, emu_wide_nce, fixed_views

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "step_call_sequences.json")
STEPS = 2
SIZE_QUERIES = ("_bytes", "_floats")


class _Proxy:
    """a library whose ``gcc_*`` symbols are logged by name as they are looked up (one look-up per call in the host layer)"""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        if name.startswith("gcc_"):
            self._log.append(name)
        return getattr(self._lib, name)


def wire(tr, log):
    """every engine of ``tr`` calls through a logging proxy; the collectives hooks log a marker"""
    seen = set()
    for eng in (tr.gin, getattr(tr, "nce", None), getattr(tr, "eng", None), getattr(tr.optimizer, "engine", None)):
        if eng is not None and id(eng) not in seen:
            seen.add(id(eng))
            eng.lib = _Proxy(eng.lib, log)
    for hook in ("_all_gather_begin", "_all_reduce", "_all_gather_end"):
        if hasattr(tr, hook):
            def logged(*a, _fn=getattr(tr, hook), _name=hook):
                log.append(f"<{_name}>")
                return _fn(*a)
            setattr(tr, hook, logged)


def _narrow(use_scalars=False, fold=True, onepass=False, collectives=False):
    if collectives:                       # tests/test_step_tail_emu._trainer(64) with the collectives switched on
        torch.manual_seed(64)
        model, ema = reference_encoder(), reference_encoder()
        ema.load_state_dict(model.state_dict())
        model._engine = ema._engine = emu_engine()
        contrast = MemoryMoCo(64, None, 96, 0.07, use_softmax=True)
        contrast._engine = emu_nce()
        tr = MoCoTrainStep(model, ema, contrast, _sampler(), posemb=lambda gr: gr, prefetch=False, collectives=True)
    else:
        tr, _ = _trainer(64)
    tr.fold, tr.onepass_head, tr.use_scalars = fold, onepass, use_scalars
    tr.dropout_seed = 0xABC
    return tr, lambda it: tr.step(it, 0.005 * (1.0 - 0.2 * it))


def _wide(masks=True, collectives=False):
    hidden = out = 66
    layers = 2
    views = [fixed_views()] * 8
    if collectives:                       # tests/test_wide_edges_emu._fused_step with the collectives switched on
        torch.manual_seed(hidden * 1000 + out)
        model, ema = encoder(hidden, out, layers), encoder(hidden, out, layers)
        ema.load_state_dict(model.state_dict())
        model._wide_engine = ema._wide_engine = emu_wide_engine()
        contrast = MemoryMoCo(out, None, 96, 0.07, use_softmax=True)
        contrast._engine = emu_wide_nce()
        tr = MoCoTrainStep(model, ema, contrast, _ScriptedSampler(views), posemb=lambda gr: gr, prefetch=False, flat_engine=emu_nce(),
                           collectives=True)
    else:
        tr = _fused_step(hidden, out, layers, views)[0]
    if masks:
        tr.mask_fn = lambda: _masks(layers, out, 5)
    torch.manual_seed(77)                 # (without injected masks the step draws them from torch's generator)
    return tr, lambda it: tr.step(it, 0.005 * (1.0 - 0.2 * it))


def _e2e(use_scalars=False):
    torch.manual_seed(1)
    model = reference_encoder()
    model._engine = emu_engine()
    tr = E2ETrainStep(model, _sampler(), posemb=lambda gr: gr, prefetch=False, engine=emu_nce())
    tr.use_scalars = use_scalars
    tr.dropout_seed = 0x1357
    return tr, lambda it: tr.step(it, 0.005 * (1.0 - 0.2 * it))


def _finetune():
    from tests.finetune_check import GOLD, batch, make_model, padded_masks
    from tests.test_finetune_emu import emu_head

    torch.manual_seed(3)                  # (the golden state leaves set2set.* / lin_readout.* at their random initialisation)
    _, _, tr = make_model("cpu", emu_engine(), emu_head())
    k = [0]

    def masks():
        k[0] += 1
        return padded_masks((k[0] - 1) % 2)

    tr.mask_fn = masks

    def step(it):
        g, y = batch(it % 2, "cpu")
        return tr.step(it, g, y, GOLD["steps"][it % 2]["lr"])

    return tr, step


CASES = {
    "narrow-by-value": lambda: _narrow(),
    "narrow-scalars-unfolded": lambda: _narrow(use_scalars=True, fold=False),
    "narrow-scalars-folded": lambda: _narrow(use_scalars=True, fold=True),
    "narrow-scalars-folded-onepass": lambda: _narrow(use_scalars=True, fold=True, onepass=True),
    "wide-66-masks": lambda: _wide(masks=True),
    "wide-66-torch-rand": lambda: _wide(masks=False),
    "e2e-by-value": lambda: _e2e(),
    "e2e-scalars": lambda: _e2e(use_scalars=True),
    "finetune": _finetune,
    "narrow-collectives": lambda: _narrow(collectives=True),
    "narrow-scalars-collectives": lambda: _narrow(use_scalars=True, collectives=True),
    "wide-66-collectives": lambda: _wide(masks=True, collectives=True),
}


def run_case(name, tmp_path, steps=STEPS):
    """-> (trainer, per-step call lists, per-step outputs) of ``steps`` steps of case ``name``"""
    group = name.endswith("collectives")
    if group:
        store = torch.distributed.FileStore(str(tmp_path / "store"), 1)
        torch.distributed.init_process_group("gloo", store=store, rank=0, world_size=1)
    try:
        tr, step = CASES[name]()
        log, calls, outs = [], [], []
        wire(tr, log)
        for it in range(steps):
            del log[:]
            outs.append(step(it))
            calls.append(list(log))
        if name == "wide-66-torch-rand":
            # where torch's generator stands after the steps: the masks are ONE torch.rand draw per step
            calls.append([f"<next torch.rand {float(torch.rand(1)):.8f}>"])
        return tr, calls, outs
    finally:
        if group:
            torch.distributed.destroy_process_group()


def _launches(calls):
    return [c for c in calls if not c.endswith(SIZE_QUERIES)]


@pytest.mark.parametrize("name", list(CASES))
def test_step_issues_the_recorded_calls_in_the_recorded_order(name, tmp_path):
    with open(FIXTURE) as f:
        want = json.load(f)[name]
    _, calls, _ = run_case(name, tmp_path)
    for it, (got, exp) in enumerate(zip(calls, want)):
        assert _launches(got) == _launches(exp), f"{name}, step {it}: launches"
        assert got == exp, f"{name}, step {it}: size queries"
    assert len(calls) == len(want)


def test_fixture_agrees_with_the_launch_lists_of_the_design_notes():
    """step 0 of the five MoCo configurations as written down when the fixture was recorded (size queries left out)"""
    with open(FIXTURE) as f:
        rec = json.load(f)
    notes = {
        "narrow-by-value": "gcc_gin_forward gcc_nce_forward gcc_nce_backward gcc_gin_backward gcc_adam_ema_step gcc_queue_enqueue",
        "narrow-scalars-unfolded": "gcc_step_scalars_fill gcc_step_scalars_fetch gcc_gin_forward gcc_nce_forward gcc_nce_backward "
                                   "gcc_gin_backward gcc_adam_ema_step_scalars gcc_queue_enqueue_scalars",
        "narrow-scalars-folded": "gcc_step_scalars_fill gcc_gin_forward_fetch gcc_nce_forward gcc_nce_backward gcc_gin_backward_sumsq "
                                 "gcc_adam_ema_enqueue_step_scalars",
        "narrow-scalars-folded-onepass": "gcc_step_scalars_fill gcc_gin_forward_fetch gcc_nce_forward_backward gcc_gin_backward_sumsq "
                                         "gcc_adam_ema_enqueue_step_scalars",
        "wide-66-masks": "gcc_ginx_forward gcc_ginx_forward gcc_ncex_forward gcc_ginx_backward gcc_adam_ema_step gcc_queue_enqueue_x",
    }
    for name, text in notes.items():
        assert _launches(rec[name][0]) == text.split(), name
