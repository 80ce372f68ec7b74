"""Device tier of the folded MoCo step: the scalars fetch inside gin_feat_kernel, the sum of squares taken in
gin_grad_final_kernel and the enqueue inside the Adam launch -- 40 launches per replayed step -- against the same step on the
separate launches (``fold=False``: 43), graph replay on, real sampler + eigensolver; and the one-pass head
(gcc_nce_forward_backward, ``onepass_head=True``: 38 launches) inside the step."""
import pytest
import torch

from tests.hipemu.emu_encoder import reference_encoder

pytestmark = pytest.mark.gpu


def test_folded_step_equals_the_step_on_the_separate_launches():
    """three steps with a learning rate above zero and in-kernel dropout; loss, prob, gradient norm step by step, the flat
    gradient, weights, Adam moments, EMA copy and queue at the end, at the tolerance of tests/test_train_step_gpu.py's "graph
    replay == eager" (rtol 1e-5, atol 1e-6).  The folded launches add nothing in another order but the clip's fp64 sum of
    squares (the norm as fp32: equal, or one ulp)."""
    a, b = _run_sides(dict(fold=False), dict(fold=True), 3)
    for key in KEYS:
        torch.testing.assert_close(b[key], a[key], rtol=1e-5, atol=1e-6, msg=lambda m, key=key: f"{key}: {m}")


def test_onepass_head_inside_the_step_first_step():
    """The one-pass head (off by default) inside the folded step against the four launches: everything ONE step computes before
    its optimiser update -- loss, prob, gradient norm, the (clipped) flat gradient -- and the queue, at the same tolerance.

    Why one step and not three: the head adds the same terms in another order, d loss / d q moves by ~1e-7 relative, and Adam's
    update g / (|g| + 1e-8) scales the elements whose gradient is rounding noise around zero (|g| 1e-12 .. 1e-9) by lr / 1e-8.
    Measured on an MI355X over three steps (rtol 1e-5 / atol 1e-6 is MISSED there): largest |one-pass - four launches| loss
    4.8e-06 (of 4.68), prob 3.3e-06, gradient norm 9.9e-04 (of 23.9, at the third step), weights 5.2e-05, exp_avg 3.7e-06;
    emulator, one step from equal weights: norms bit-equal, largest gradient difference 2.2e-08 (of 0.099), 33 of 61,904 weights
    more than 1e-6 apart (up to 2.9e-05), all at |g| < 1e-9.  That is why the trainer does not take this head unless asked to
    (profiles/step_fold_dump_diff.txt)."""
    a, b = _run_sides(dict(fold=True, onepass_head=False), dict(fold=True, onepass_head=True), 1)
    for key in ("loss", "prob", "gnorm", "grad", "mem"):
        torch.testing.assert_close(b[key], a[key], rtol=1e-5, atol=1e-6, msg=lambda m, key=key: f"{key}: {m}")


KEYS = ("loss", "prob", "gnorm", "grad", "flat", "ema", "mem", "m", "v")


def _run_sides(kw_a, kw_b, STEPS):
    from gcc_amd.contrast import MemoryMoCo
    from gcc_amd.graph import DeviceGraph
    from gcc_amd.graphgen import powerlaw_graph
    from gcc_amd.posemb import DevicePosEmb
    from gcc_amd.sampler import DeviceRWRSampler
    from gcc_amd.train_step import MoCoTrainStep

    rp, ci = powerlaw_graph(50_000, 500_000, 3)
    graph = DeviceGraph(rp, ci, rw_hops=64, device="cuda:0")
    B, K, CHUNK, DEPTH = 32, 96, 2, 2
    sides = []
    for kw in (kw_a, kw_b):
        torch.manual_seed(4)
        model, ema = reference_encoder().cuda(), reference_encoder().cuda()
        ema.load_state_dict(model.state_dict())
        contrast = MemoryMoCo(64, None, K, 0.07, use_softmax=True).cuda()
        smp = DeviceRWRSampler(graph, B, run_seed=9, num_buffers=DEPTH * CHUNK, max_steps=CHUNK)
        pe = DevicePosEmb(B, smp.node_cap, 32, device="cuda:0", seed=9, num_buffers=DEPTH * CHUNK, max_views=2 * CHUNK)
        tr = MoCoTrainStep(model, ema, contrast, smp, pe, depth=DEPTH, chunk=CHUNK, prefetch=True, graph=True, **kw)
        assert tr.fold == kw["fold"] and tr.onepass_head == kw.get("onepass_head", False)
        tr.dropout_seed = 77
        losses, probs, gnorms = [], [], []
        for i in range(STEPS):
            out = tr.step(i, 0.005 * (1.0 - 0.03 * i))
            losses.append(out["loss"].reshape(()).clone())
            probs.append(out["prob"].reshape(()).clone())
            gnorms.append(torch.as_tensor(out["grad_norm"]).reshape(()).clone())
        torch.cuda.synchronize()
        assert tr.check_status(strict_posemb=True) == 0
        assert tr.graph_replays == STEPS - 1 and int(tr.ring_counter) == STEPS
        sides.append(dict(loss=torch.stack(losses).cpu(), prob=torch.stack(probs).cpu(), gnorm=torch.stack(gnorms).cpu(),
                          grad=tr.flat_grad.cpu(), flat=tr.flat.cpu(), ema=tr.flat_ema.cpu(), mem=contrast.memory.cpu(),
                          m=tr.optimizer.exp_avg.cpu(), v=tr.optimizer.exp_avg_sq.cpu(), index=contrast.index))
    a, b = sides
    assert a["index"] == b["index"] == (STEPS * B) % K
    assert torch.isfinite(b["loss"]).all() and float(b["gnorm"].min()) > 0
    for key in KEYS:
        d = (b[key] - a[key]).abs()
        print(f"{key}: largest |difference| {float(d.max()):.3e} (largest |value| {float(a[key].abs().max()):.3e})")
    return a, b
