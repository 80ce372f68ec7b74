"""--optimizer sgd / adagrad on the data-parallel MoCo step, on CPU: two processes over gloo run
``MoCoTrainStep(optimizer=...)`` (emulator kernels) on different seed-batch shards.  The assertions
tests/test_multi_gpu_gloo.py makes for Adam at two ranks: identical weights, EMA weights, queue and gradient on both ranks;
the gradient is the mean of the two shards' single-process gradients and the keys sit in rank order, at that test's
tolerances -- and the weights are the rule's single-process step on that mean gradient (the tail takes 1 / world as its
grad_scale)."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

GOLD_PATH = os.path.join(os.path.dirname(__file__), "golden", "encoder_golden.pt")
RULE = dict(sgd=dict(momentum=0.9), adagrad=dict(lr_decay=0.01))
LR = dict(sgd=0.1, adagrad=0.005)


def _build(rule, rank_views, world, rank):
    from gcc_amd.contrast import MemoryMoCo
    from gcc_amd.train_step import MoCoTrainStep
    from tests.hipemu.emu_encoder import CpuBatch, emu_engine, reference_encoder
    from tests.test_nce_emu import emu_nce

    gold = torch.load(GOLD_PATH, weights_only=False)
    g = gold["moco"]
    model, ema = reference_encoder(), reference_encoder()
    model.load_state_dict(g["init"]["model"])
    ema.load_state_dict(g["init"]["model_ema"])
    model._engine = ema._engine = emu_engine()
    contrast = MemoryMoCo(64, None, g["K"], g["T"], use_softmax=True)
    contrast._engine = emu_nce()
    contrast.memory.copy_(g["init"]["memory"])

    class Stub:
        batch_size = 6

        def sample(self, first_id, prof=None):
            return CpuBatch(gold["views"][rank_views[0]]), CpuBatch(gold["views"][rank_views[1]])

    step = MoCoTrainStep(model, ema, contrast, Stub(), posemb=lambda gr, prof=None: gr, prefetch=False, world_size=world, rank=rank,
                         clip_norm=0.0, optimizer=rule, **RULE[rule])          # raw gradients: clipping is nonlinear
    masks = g["masks"].contiguous()
    step.mask_fn = lambda: masks
    return step, model, ema, contrast


def _worker(rank, world, port, out_dir, rule):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        step, model, ema, contrast = _build(rule, (0, 1) if rank == 0 else (1, 0), world, rank)      # different shards
        assert step.collectives and step.optimizer.rule == rule
        out = step.step(0, LR[rule])
        torch.save(dict(model=model.state_dict(), ema=ema.state_dict(), memory=contrast.memory.clone(), index=contrast.index,
                        grad=step.flat_grad.clone(), state=step.optimizer.state.clone(), live=step.live.clone(),
                        loss=out["loss"].clone()),
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("rule", ["sgd", "adagrad"])
def test_two_rank_step_over_gloo(tmp_path, rule):
    port = 29500 + (os.getpid() + (13 if rule == "sgd" else 29)) % 1000
    mp.spawn(_worker, args=(2, port, str(tmp_path), rule), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=False)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=False)
    stats = lambda k: "running_" in k or "num_batches" in k  # noqa: E731  (BatchNorm statistics are per rank)
    for k in r0["model"]:                                # identical replicas after the step
        if not stats(k):
            torch.testing.assert_close(r0["model"][k], r1["model"][k], rtol=0, atol=0, msg=k)
            torch.testing.assert_close(r0["ema"][k], r1["ema"][k], rtol=0, atol=0, msg=k)
    for key in ("memory", "grad", "state"):
        torch.testing.assert_close(r0[key], r1[key], rtol=0, atol=0, msg=key)
    assert r0["index"] == r1["index"] == 12              # 2 ranks x 6 keys enqueued
    # single-process references for each shard: averaged gradient and rank-ordered keys
    grads, keys = [], []
    for views in ((0, 1), (1, 0)):
        step, model, ema, contrast = _build(rule, views, 1, 0)
        step.step(0, LR[rule])
        grads.append(step.flat_grad.clone())
        keys.append(contrast.memory[:6].clone())
    mean = (grads[0] + grads[1]) / 2
    torch.testing.assert_close(r0["grad"], mean, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(r0["memory"][:6], keys[0], rtol=1e-6, atol=1e-7)      # rank 0's keys first
    torch.testing.assert_close(r0["memory"][6:12], keys[1], rtol=1e-6, atol=1e-7)    # then rank 1's
    # the rule's own single-process step on the mean gradient, from the initial weights
    step, model, ema, contrast = _build(rule, (0, 1), 1, 0)
    init = step.live.clone()
    step.flat_grad.copy_(mean)
    step.optimizer.param_groups[0]["lr"] = LR[rule]
    step.optimizer.step()
    # Adagrad divides a gradient by its own size: entries whose true gradient is zero (biases in front of a BatchNorm) hold rounding
    # noise that it turns into a move of up to +-lr -- those are held to the size of the step, as tests/finetune_check.py holds Adam's
    solid = mean.abs() >= 1e-7 if rule == "adagrad" else torch.ones_like(mean, dtype=torch.bool)
    assert torch.all((r0["live"] - step.live).abs()[~solid] <= 2 * LR[rule])
    torch.testing.assert_close(r0["live"][solid], step.live[solid], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(r0["state"][solid], step.optimizer.state[solid], rtol=1e-5, atol=1e-7)
    assert float((step.live - init).abs().max()) > 1e-3 and int(solid.sum()) > 50000
