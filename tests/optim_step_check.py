"""MoCoTrainStep / E2ETrainStep / FinetuneTrainStep with ``optimizer="sgd"`` and ``"adagrad"`` against the API composition of the
same kernels -- autograd through GraphEncoder.forward and the heads, clip_grad_norm_ / clip_grad_value_, torch.optim,
moment_update: what ``train.py --step-path api`` runs -- over three steps from the same initial weights, batches and injected
dropout keep-masks.  Shared by tests/test_optim_step_emu.py (emulator build, CPU tensors) and tests/test_optim_step_gpu.py
(gfx950 library, cuda:0).  Tolerances: those of the Adam step checks (tests/test_train_step_emu.py, tests/finetune_check.py)."""
import io
import os
from unittest import mock

import torch
import torch.nn as nn

from gcc_amd.contrast import MemoryMoCo, NceEngine, NCESoftmaxLoss, NCESoftmaxLossNS, e2e_logits
from gcc_amd.finetune import ClsHeadEngine, FinetuneTrainStep, clear_bn, cls_head_loss
from gcc_amd.train_step import (E2ETrainStep, FlatAdagrad, FlatSGD, MoCoTrainStep, clip_grad_norm, flatten_parameters,
                                moment_update)
from tests import finetune_check as F
from tests.hipemu.emu_encoder import CpuBatch, reference_encoder
from tests.wide_edges_check import EMU, GPU, ScriptedSampler, encoder, hand_batch  # noqa: F401  (the tiers)

GOLD = torch.load(os.path.join(os.path.dirname(__file__), "golden", "encoder_golden.pt"), weights_only=False)
WEIGHTS = dict(rtol=1e-3, atol=2e-5)         # parameters, EMA parameters, BatchNorm running statistics
QUEUE = dict(rtol=1e-4, atol=2e-5)
LOSS = dict(rtol=1e-4, atol=1e-5)
GNORM = dict(rtol=1e-3, atol=1e-5)
STEPS, WD, CLIP, ALPHA = 3, 1e-5, 1.0, 0.999
RULE = dict(sgd=dict(momentum=0.9), adagrad=dict(lr_decay=0.01))
BASE_LR = dict(sgd=0.1, adagrad=0.005)       # SGD's update is lr x a gradient of norm <= 1: a rate at which it clears the atol


def lr_of(rule, it):
    return BASE_LR[rule] * (1.0 - 0.2 * it)


def narrow_engines(tier):
    """(encoder engine, head engine, fine-tuning head engine) of the 64-channel kernels; None = the gfx950 library's"""
    if tier.name == "gpu":
        return None, None, None
    from tests.hipemu.emu_driver import emu_lib
    from tests.hipemu.emu_encoder import emu_engine

    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    return emu_engine(), NceEngine(lib=emu_lib(), ptr=ptr), ClsHeadEngine(lib=emu_lib(), ptr=ptr)


def torch_optimizer(rule, params, lr):
    if rule == "sgd":
        return torch.optim.SGD(params, lr=lr, momentum=RULE[rule]["momentum"], weight_decay=WD)
    return torch.optim.Adagrad(params, lr=lr, lr_decay=RULE[rule]["lr_decay"], weight_decay=WD)


class rand_returns:
    """the API path draws its dropout keep-masks with torch.rand: the next draws are ``masks`` (thresholded back to themselves)"""

    def __init__(self, *masks):
        self.masks = list(masks)

    def __enter__(self):
        self.patch = mock.patch.object(torch, "rand", lambda *a, **k: self.masks.pop(0).clone())
        self.patch.__enter__()

    def __exit__(self, *exc):
        self.patch.__exit__(*exc)
        assert not self.masks


def keep_masks(tier, n, rows, cols, seed, layers=5):
    gen = torch.Generator().manual_seed(seed)
    return [tier.to((torch.rand(layers, rows, cols, generator=gen) >= 0.5).float().contiguous()) for _ in range(n)]


def close(what, got, ref, tol):
    torch.testing.assert_close(got.detach().cpu(), ref.detach().cpu(), msg=lambda m: f"{what}: {m}", **tol)


class NoiseEntries:
    """Adagrad, like Adam, divides a gradient by its own size: an entry whose true gradient is zero (a Linear bias in front of a
    BatchNorm) carries rounding noise of ~1e-10 that the rule turns into a move of up to +-clr, with whatever sign the noise has.
    As tests/finetune_check.py::check_steps does for Adam, entries whose reference gradient has been below 1e-7 are held to the
    size of the steps taken (twice the sum of the rates so far), every other entry to the usual tolerance."""

    def __init__(self, rule, model):
        self.on, self.model, self.mask, self.rates = rule == "adagrad", model, {}, 0.0

    def after_backward(self, lr):
        """call between the reference's backward and its optimizer step"""
        self.rates += lr
        if self.on:
            for n, p in self.model.named_parameters():
                if p.grad is not None:
                    small = (p.grad.abs() < 1e-7).cpu()
                    self.mask[n] = self.mask[n] | small if n in self.mask else small


def same_modules(what, got, ref, moved_from=None, noise=None):
    """every state_dict entry (parameters and BatchNorm running statistics); ``moved_from``: the initial state -- the weights
    must have moved away from it by more than the tolerance, or the comparison would hold for a step that did nothing"""
    a, b = got.state_dict(), ref.state_dict()
    assert set(a) == set(b)
    for k in a:
        x, y = a[k].detach().cpu(), b[k].detach().cpu()
        m = noise.mask.get(k) if noise is not None else None
        if m is not None and m.any():
            assert torch.all((x - y).abs()[m] <= 2 * noise.rates), f"{what} {k}: a noise entry moved by more than the steps taken"
            x, y = x[~m], y[~m]
        close(f"{what} {k}", x, y, WEIGHTS)
    if moved_from is not None:
        moved = max(float((a[k].cpu() - moved_from[k]).abs().max()) for k in a if a[k].is_floating_point())
        assert moved > 50 * WEIGHTS["atol"], f"{what}: the largest move of a weight is {moved:.2e}"


class StubSampler:
    def __init__(self, views):
        self.views, self.batch_size = views, views[0].batch_size

    def sample(self, first_id, prof=None):
        return self.views


def golden_views(tier):
    return tuple(tier.batch(CpuBatch(GOLD["views"][i])) for i in range(2))


# ------------------------------------------------------------------------------------------------------------------- MoCo
def moco_side(tier, rule, wide, fused):
    """(trainer or None, model, ema, contrast, views) of one side; both sides start from the same weights and queue"""
    gin, nce, _ = narrow_engines(tier)
    if wide:                                                   # hidden 128: the any-width kernels, scalars by value
        torch.manual_seed(128)
        model, ema = encoder(128, 128, 2), encoder(128, 128, 2)
        contrast = MemoryMoCo(128, None, 96, 0.07, use_softmax=True)
        views = (hand_batch(260, 300, 1, tier=tier), hand_batch(250, 300, 2, tier=tier))
        sampler = ScriptedSampler([views] * STEPS)
    else:
        g = GOLD["moco"]
        model, ema = reference_encoder(), reference_encoder()
        model.load_state_dict(g["init"]["model"])
        contrast = MemoryMoCo(64, None, g["K"], g["T"], use_softmax=True)
        contrast.memory.copy_(g["init"]["memory"])
        views = golden_views(tier)
        sampler = StubSampler(views)
    ema.load_state_dict(model.state_dict())
    model, ema, contrast = tier.to(model), tier.to(ema), tier.to(contrast)
    if wide:
        model._wide_engine = ema._wide_engine = tier.wide_engine()
        contrast._engine = tier.wide_nce()
    elif gin is not None:
        model._engine = ema._engine = gin
        contrast._engine = nce
    tr = None
    if fused:
        tr = MoCoTrainStep(model, ema, contrast, sampler, posemb=lambda gr, prof=None: gr, prefetch=False, weight_decay=WD,
                           clip_norm=CLIP, alpha=ALPHA, optimizer=rule, flat_engine=tier.flat_engine() if wide else None,
                           **RULE[rule])
        assert tr.wide == wide and isinstance(tr.optimizer, FlatSGD if rule == "sgd" else FlatAdagrad)
    else:                                                      # train.py's API branch
        flatten_parameters(model)
        flatten_parameters(ema)
        model.train()
        ema.eval()
        for mod in ema.modules():
            if isinstance(mod, nn.BatchNorm1d):
                mod.train()
    return tr, model, ema, contrast, views


def check_moco(tier, rule, wide=False):
    trf, mf, ef, cf, _ = moco_side(tier, rule, wide, fused=True)
    _, ma, ea, ca, (q, k) = moco_side(tier, rule, wide, fused=False)
    init = {kk: v.detach().cpu().clone() for kk, v in ma.state_dict().items()}
    flat_eng = tier.flat_engine() if wide or tier.name == "gpu" else narrow_engines(tier)[1]
    opt = torch_optimizer(rule, ma.parameters(), BASE_LR[rule])
    cols = 128 if wide else 64
    masks = keep_masks(tier, STEPS, q.batch_size, cols, 3, layers=len(mf.gnn.ginlayers) + 1)
    crit = NCESoftmaxLoss()
    noise = NoiseEntries(rule, ma)
    for it in range(STEPS):
        lr = lr_of(rule, it)
        trf.mask_fn = lambda it=it: masks[it]
        out = trf.step(it, lr)
        with rand_returns(masks[it]):                          # train.py:245-262
            feat_q = ma(q)
        with torch.no_grad():
            feat_k = ea(k)
        logits = ca(feat_q, feat_k)
        opt.zero_grad()
        loss = crit(logits)
        loss.backward()
        gn = clip_grad_norm(list(ma.parameters()), CLIP)
        noise.after_backward(lr)
        for grp in opt.param_groups:
            grp["lr"] = lr
        opt.step()
        moment_update(ma, ea, ALPHA, engine=flat_eng)
        tier.sync()
        what = f"moco {rule}{' wide' if wide else ''} step {it}"
        close(f"{what} loss", out["loss"].reshape(()), loss.reshape(()), LOSS)
        close(f"{what} grad norm", torch.as_tensor(out["grad_norm"]).reshape(()), torch.as_tensor(gn).reshape(()), GNORM)
        same_modules(f"{what} model", mf, ma, init if it == STEPS - 1 else None, noise)
        same_modules(f"{what} model_ema", ef, ea)
        close(f"{what} queue", cf.memory, ca.memory, QUEUE)
        assert cf.index == ca.index == ((it + 1) * q.batch_size) % cf.queueSize
    assert trf.optimizer.steps == STEPS and trf.optimizer.param_groups[0]["lr"] == lr_of(rule, STEPS - 1)
    acc = trf.meter_acc.tolist()
    assert acc[4] == STEPS and acc[3] == STEPS * (int(q.node_off[q.batch_size]) + int(k.node_off[k.batch_size]))


# -------------------------------------------------------------------------------------------------------------------- E2E
def check_e2e(tier, rule):
    gin, nce, _ = narrow_engines(tier)
    sides = []
    for _ in range(2):
        model = reference_encoder()
        model.load_state_dict(GOLD["e2e"]["init"]["model"])
        model = tier.to(model)
        if gin is not None:
            model._engine = gin
        sides.append(model)
    mf, ma = sides
    q, k = views = golden_views(tier)
    trf = E2ETrainStep(mf, StubSampler(views), posemb=lambda gr, prof=None: gr, prefetch=False, engine=nce, weight_decay=WD,
                       clip_norm=CLIP, optimizer=rule, **RULE[rule])
    assert isinstance(trf.optimizer, FlatSGD if rule == "sgd" else FlatAdagrad)
    flatten_parameters(ma)
    ma.train()
    init = {kk: v.detach().cpu().clone() for kk, v in ma.state_dict().items()}
    opt = torch_optimizer(rule, ma.parameters(), BASE_LR[rule])
    mq, mk = keep_masks(tier, STEPS, q.batch_size, 64, 5), keep_masks(tier, STEPS, q.batch_size, 64, 6)
    crit = NCESoftmaxLossNS()
    noise = NoiseEntries(rule, ma)
    for it in range(STEPS):
        lr = lr_of(rule, it)
        trf.mask_fn = lambda it=it: (mq[it], mk[it])
        out = trf.step(it, lr)
        with rand_returns(mq[it], mk[it]):                     # train.py:245-260
            feat_q = ma(q)
            feat_k = ma(k)
        logits = e2e_logits(feat_q, feat_k, trf.T, engine=nce)
        opt.zero_grad()
        loss = crit(logits)
        loss.backward()
        gn = clip_grad_norm(list(ma.parameters()), CLIP)
        noise.after_backward(lr)
        for grp in opt.param_groups:
            grp["lr"] = lr
        opt.step()
        tier.sync()
        what = f"e2e {rule} step {it}"
        close(f"{what} loss", out["loss"].reshape(()), loss.reshape(()), LOSS)
        close(f"{what} grad norm", torch.as_tensor(out["grad_norm"]).reshape(()), torch.as_tensor(gn).reshape(()), GNORM)
        same_modules(f"{what} model", mf, ma, init if it == STEPS - 1 else None, noise)
    assert trf.optimizer.steps == STEPS


# -------------------------------------------------------------------------------------------------------------- fine-tuning
def check_finetune(tier, rule):
    """golden batch 0 (six graphs), batch 1 (four graphs padded with two empty ones), batch 0 again; the encoder's optimizer is
    ``rule``, the head's stays Adam on both sides"""
    gin, _, head_eng = narrow_engines(tier)
    dev = tier.device
    sides = []
    for _ in range(2):
        model, head = F.golden_encoder(), nn.Linear(64, 3)
        model.load_state_dict(F.GOLD["init"]["model"], strict=False)      # (the golden file has no set2set / lin_readout weights:
        if sides:                                                         #  the second side takes the first side's)
            model.load_state_dict(sides[0][0].state_dict())
        head.load_state_dict(F.GOLD["init"]["head"])
        model, head = tier.to(model), tier.to(head)
        if gin is not None:
            model._engine = gin
        sides.append((model, head))
    (mf, hf), (ma, ha) = sides
    trf = FinetuneTrainStep(mf, hf, weight_decay=WD, clip_value=1.0, engine=head_eng, optimizer=rule, **RULE[rule])
    assert trf.optimizer.rule == rule and "betas" in trf.head_optimizer.param_groups[0]      # the head's optimizer: Adam
    flatten_parameters(ma)
    clear_bn(mf)
    clear_bn(ma)
    init = {kk: v.detach().cpu().clone() for kk, v in ma.state_dict().items()}
    opt = torch_optimizer(rule, ma.parameters(), BASE_LR[rule])
    hopt = torch.optim.Adam(ha.parameters(), lr=BASE_LR[rule], betas=(0.9, 0.999), weight_decay=WD)
    noise = NoiseEntries(rule, ma)
    for it, i in enumerate((0, 1, 0)):
        lr = lr_of(rule, it)
        g, y = F.batch(i, dev)
        keep = F.padded_masks(i).to(dev)
        trf.mask_fn = lambda keep=keep: keep
        out = trf.step(it, g, y, lr)
        ma.train()                                              # finetune_main.train_finetune's API branch
        with rand_returns(keep):
            feat_q = ma(g)
        loss, _logits, correct = cls_head_loss(feat_q, ha, y, engine=head_eng)
        opt.zero_grad()
        hopt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_value_(ma.parameters(), 1)
        torch.nn.utils.clip_grad_value_(ha.parameters(), 1)
        noise.after_backward(lr)
        for o in (opt, hopt):
            for grp in o.param_groups:
                grp["lr"] = lr
        opt.step()
        hopt.step()
        tier.sync()
        what = f"finetune {rule} step {it}"
        close(f"{what} loss", out["loss"].reshape(()), loss.reshape(()), LOSS)
        assert out["correct"].tolist() == correct.tolist()
        same_modules(f"{what} model", mf, ma, init if it == 2 else None, noise)
        close(f"{what} head weight", hf.weight, ha.weight, dict(rtol=1e-4, atol=2e-6))
        close(f"{what} head bias", hf.bias, ha.bias, dict(rtol=1e-4, atol=2e-6))
    assert trf.optimizer.steps == trf.head_optimizer.steps == 3


# ------------------------------------------------------------------------------------------------- the optimizer objects
def check_state_dict_and_param_group_lr(tier, rule):
    """``state_dict()`` survives torch.save / torch.load; a rate the caller writes into ``param_groups[0]["lr"]`` is the rate
    of the next step (train.py sets it every step, adjust_learning_rate rewrites it)"""
    n = 300
    gen = torch.Generator().manual_seed(7)
    p0, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.01
    p, grad = tier.to(p0.clone()), tier.to(g.clone())
    eng = tier.flat_engine()
    if rule == "sgd":
        opt = FlatSGD(p, grad, 0.5, 0.9, 0.0, 1.0, eng)
        assert set(opt.param_groups[0]) == {"lr", "momentum", "weight_decay"}
    else:
        opt = FlatAdagrad(p, grad, 0.5, 0.01, 0.0, 1.0, eng)
        assert set(opt.param_groups[0]) == {"lr", "lr_decay", "eps", "weight_decay"}
    opt.param_groups[0]["lr"] = 0.125
    opt.step()
    tier.sync()
    ref = p0 - 0.125 * (g if rule == "sgd" else g / (g.abs() + 1e-10))          # the first step of either rule, unclipped
    close(f"{rule}: the caller's rate", p, ref, dict(rtol=1e-5, atol=1e-7))
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=False)
    assert sd["param_groups"] == opt.param_groups and sd["state"]["step"] == 1
    key = "momentum_buffer" if rule == "sgd" else "sum"
    assert set(sd["state"]) == {"step", key} and torch.equal(sd["state"][key].cpu(), opt.state.cpu())
    assert float(sd["state"][key].abs().max()) > 0


# ----------------------------------------------------------------------------------------------- graph replay (device only)
def check_graph_replay_gives_the_eager_bits(rule):
    """The 64-channel MoCo step on the real producer (one lane, depth 2, chunks of two steps: four ring slots) over ten steps:
    with ``graph=True`` every slot is replayed at least once, and parameters, optimizer state, EMA copy and queue end with the
    bits of the ``graph=False`` run.  For Adagrad with lr_decay 0.01 that holds only if every step's clr travels through the
    scalars ring."""
    from gcc_amd.graph import DeviceGraph
    from gcc_amd.graphgen import powerlaw_graph
    from gcc_amd.posemb import DevicePosEmb
    from gcc_amd.sampler import DeviceRWRSampler

    rp, ci = powerlaw_graph(20_000, 200_000, 3)
    graph = DeviceGraph(rp, ci, rw_hops=32, device="cuda:0")
    B, K, CHUNK, DEPTH, N = 16, 96, 2, 2, 10
    sides = []
    for use_graph in (False, True):
        torch.manual_seed(4)
        model, ema = reference_encoder().cuda(), reference_encoder().cuda()
        ema.load_state_dict(model.state_dict())
        contrast = MemoryMoCo(64, None, K, 0.07, use_softmax=True).cuda()
        smp = DeviceRWRSampler(graph, B, run_seed=9, num_buffers=DEPTH * CHUNK, max_steps=CHUNK)
        pe = DevicePosEmb(B, smp.node_cap, 32, device="cuda:0", seed=9, num_buffers=DEPTH * CHUNK, max_views=2 * CHUNK)
        tr = MoCoTrainStep(model, ema, contrast, smp, pe, depth=DEPTH, chunk=CHUNK, prefetch=True, graph=use_graph, optimizer=rule,
                           **RULE[rule])
        tr.dropout_seed = 77
        for i in range(N):
            tr.step(i, lr_of(rule, 0) * (1.0 - 0.03 * i))
        torch.cuda.synchronize()
        assert tr.check_status(strict_posemb=True) == 0 and tr.optimizer.steps == N
        if use_graph:
            assert len(tr.graphs) == DEPTH * CHUNK and tr.graph_replays >= N - DEPTH * CHUNK > DEPTH * CHUNK
            assert int(tr.ring_counter) == N
        else:
            assert tr.graph_replays == 0
        sides.append(dict(flat=tr.flat.cpu(), state=tr.optimizer.state.cpu(), ema=tr.flat_ema.cpu(), queue=contrast.memory.cpu(),
                          grad=tr.flat_grad.cpu(), index=contrast.index))
    a, b = sides
    assert a["index"] == b["index"] == (N * B) % K
    for key in ("flat", "state", "ema", "queue", "grad"):
        assert torch.isfinite(a[key]).all()
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), f"{rule}: {key} differs between replay and eager"
