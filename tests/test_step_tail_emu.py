"""The folded tail and head-of-stream of the single-GPU MoCo step on the wave64 emulator:
  * gin_grad_final_kernel's sum-of-squares partials (gcc_gin_backward_sumsq) + Adam-with-partials
    (gcc_adam_ema_enqueue_step_scalars) against gcc_adam_ema_step on the same gradient, at hidden 64 and 32;
  * the enqueue inside the Adam launch against gcc_queue_enqueue_scalars, wrap-around included;
  * the scalars fetch inside gin_feat_kernel (gcc_gin_forward_fetch) against gcc_step_scalars_fetch."""
import numpy as np
import pytest
import torch

from gcc_amd.contrast import MemoryMoCo
from gcc_amd.train_step import MoCoTrainStep
from tests.hipemu.emu_encoder import emu_engine, reference_encoder
from tests.test_headline_step_emu import B, OracleSampler
from tests.test_hidden_size_emu import narrow_encoder
from tests.test_nce_emu import emu_nce


_SAMPLER = []


def _sampler():
    """ONE sampled batch for every trainer of this file (the SciPy positional embedding of a fresh one differs in its last bits)"""
    if not _SAMPLER:
        _SAMPLER.append(OracleSampler())
    return _SAMPLER[0]


def _trainer(hidden):
    torch.manual_seed(hidden)
    model, ema = (reference_encoder(), reference_encoder()) if hidden == 64 else (narrow_encoder(hidden, hidden), narrow_encoder(hidden, hidden))
    ema.load_state_dict(model.state_dict())
    model._engine = ema._engine = emu_engine()
    contrast = MemoryMoCo(hidden, None, 96, 0.07, use_softmax=True)
    contrast._engine = emu_nce()
    return MoCoTrainStep(model, ema, contrast, _sampler(), posemb=lambda gr: gr, prefetch=False), model


def _ulps(a, b):
    ia, ib = np.float32(a).view(np.int32), np.float32(b).view(np.int32)
    return abs(int(ia) - int(ib))


@pytest.mark.parametrize("hidden", [64, 32])
@pytest.mark.parametrize("dscale", [40.0, 0.001])       # gradient norm above the clip (1.0) / below it
def test_partials_and_adam_with_partials_equal_the_separate_norm_launch(hidden, dscale):
    tr, model = _trainer(hidden)
    nce, gin = tr.nce, tr.gin
    q, _ = _sampler().views
    p, buf = gin.make_pass(model, q, training=True, keep=None, dropout_seed=5)
    gin.forward([p])
    dfeat = torch.randn(B, 64) * dscale
    if hidden < 64:
        dfeat[:, hidden:] = 0.0
    parts = torch.full((4096,), float("nan"), dtype=torch.float64)
    _, n = gin.backward(model, p, buf, dfeat, targets=tr.grad_views, sumsq=parts)
    assert 0 < n <= parts.numel() and torch.isfinite(parts[:n]).all() and torch.isnan(parts[n:]).all()
    grad = tr.flat_grad.clone()
    # what the kernel stored is all there is in the flat buffer: the partials add up to the buffer's squared norm.  At hidden 32
    # the buffer holds zero-padded blocks; elements the kernel does not store must be exactly zero for this to hold.
    full = float(grad.double().pow(2).sum())
    assert abs(float(parts[:n].sum()) - full) <= 1e-12 * full
    assert (float(full) ** 0.5 > 1.0) == (dscale > 1.0)
    # the same backward without the partials stores the same gradient, bit for bit
    tr.flat_grad.zero_()
    gin.backward(model, p, buf, dfeat, targets=tr.grad_views)
    assert torch.equal(tr.flat_grad, grad)

    lr, betas, steps = 0.004, (0.9, 0.999), 3
    scalars = torch.zeros(24, dtype=torch.uint8)
    nce.set_scalars(scalars, lr, betas, steps, 0, 0)
    sides = []
    for folded in (False, True):
        flat, ema = tr.flat.clone(), tr.flat_ema.clone()
        g = grad.clone()
        torch.manual_seed(1)
        m, v = torch.rand_like(g) * 1e-3, torch.rand_like(g) * 1e-6
        gn = torch.zeros(1)
        scratch = torch.zeros(64, dtype=torch.float64)
        kw = dict(stream=None, ema=ema, ema_src=flat, ema_m=0.999)
        if folded:
            nce.adam_ema(flat[: tr.n_live], g, m, v, lr, betas, 1e-8, 1e-5, steps, 1.0, gn, scratch, scalars=scalars,
                         sumsq_parts=(parts, n), **kw)
        else:
            nce.adam_ema(flat[: tr.n_live], g, m, v, lr, betas, 1e-8, 1e-5, steps, 1.0, gn, scratch, **kw)
        sides.append((gn, flat, ema, m, v, g))
    gn_a, gn_b = float(sides[0][0]), float(sides[1][0])
    print(f"hidden {hidden}: grad_norm separate {gn_a!r} folded {gn_b!r}")
    assert _ulps(gn_a, gn_b) <= 1                    # the same squares added in fp64 in another order
    for a, b in zip(sides[0][1:], sides[1][1:]):
        if gn_a == gn_b:                             # tests/test_train_step_emu.py's tolerance for gcc_adam_ema_step: none
            torch.testing.assert_close(a, b, rtol=0, atol=0)
        else:                                        # a clip coefficient one ulp apart: its FlatAdam tolerance
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    assert not torch.equal(sides[1][5], grad) or dscale < 1.0      # (clipped: the clipped gradient was left in the buffer)


@pytest.mark.parametrize("index,nkeys,K", [(0, 6, 96), (93, 6, 96), (90, 6, 96), (5, 96, 96), (40, 70, 100)])
def test_enqueue_inside_the_adam_launch(index, nkeys, K):
    """queue rows bit-equal to gcc_queue_enqueue_scalars', wrap-around (index + nkeys > K) included; Adam's results untouched
    by the extra workgroups"""
    nce = emu_nce()
    torch.manual_seed(index + nkeys)
    mem0, keys = torch.randn(K, 64), torch.randn(nkeys, 64)
    scalars = torch.zeros(24, dtype=torch.uint8)
    nce.set_scalars(scalars, 0.003, (0.9, 0.999), 2, index, 0)
    ref = mem0.clone()
    nce.enqueue(ref, keys, index, scalars=scalars)
    expect = mem0.clone()
    expect[(index + torch.arange(nkeys)) % K] = keys
    assert torch.equal(ref, expect)
    n = 1000
    sides = []
    for folded in (False, True):
        mem = mem0.clone()
        p, g = torch.linspace(-1, 1, n), torch.sin(torch.arange(n, dtype=torch.float32))
        m, v, gn = torch.zeros(n), torch.zeros(n), torch.zeros(1)
        scratch = torch.zeros(64, dtype=torch.float64)
        nce.adam_ema(p, g, m, v, 0.0, (0.9, 0.999), 1e-8, 1e-5, 0, 1.0, gn, scratch, scalars=scalars,
                     **(dict(enqueue=(mem, keys)) if folded else {}))
        if not folded:
            nce.enqueue(mem, keys, index, scalars=scalars)
        sides.append((mem, p, g, m, v, gn))
    for a, b in zip(*sides):
        assert torch.equal(a, b)
    assert torch.equal(sides[1][0], expect)


def test_scalars_fetch_inside_gin_feat(monkeypatch):
    """the device struct's bytes and the step counter after 1, 2 and ring_len + 1 steps equal gcc_step_scalars_fetch's; the
    forward's outputs are those of gcc_gin_forward after a separate fetch (the readout reads the dropout key from the struct)"""
    tr, model = _trainer(64)
    nce, gin = tr.nce, tr.gin
    ring_len = 3
    ring = torch.zeros(24 * ring_len, dtype=torch.uint8)
    q, k = _sampler().views
    state = []
    for folded in (False, True):
        scalars, counter = torch.zeros(24, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
        seen = []
        for step in range(ring_len + 2):
            nce.fill_scalars(ring, step % ring_len, 0.001 * (step + 1), (0.9, 0.999), step + 1, 7 * step, 0xC0FFEE + step)
            pq, bufq = gin.make_pass(model, q, training=True, keep=None, slot=("t", 0), dropout_seed=0, scalars=scalars)
            pk, bufk = gin.make_pass(tr.ema, k, training=True, keep=None, slot=("t", 1), backward=False)
            if folded:
                gin.forward([pq, pk], fetch=(scalars, ring, ring_len, counter))
            else:
                nce.fetch_scalars(scalars, ring, ring_len, counter)
                gin.forward([pq, pk])
            assert bytes(scalars.numpy()) == bytes(ring[24 * (step % ring_len): 24 * (step % ring_len + 1)].numpy())
            seen.append((scalars.clone(), int(counter), bufq["feat"].clone(), bufk["feat"].clone()))
        state.append(seen)
    for step, (a, b) in enumerate(zip(*state)):
        assert torch.equal(a[0], b[0]) and a[1] == b[1] == step + 1
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    feats = [s[2] for s in state[1]]
    assert not torch.equal(feats[0], feats[1])         # (the dropout key of the fetched entry is really used)


@pytest.mark.parametrize("onepass", [False, True])
def test_folded_step_equals_the_separate_launches_on_the_emulator(onepass, monkeypatch):
    """MoCoTrainStep with device-resident scalars, folded (``onepass``: with the one-pass head as well) against ``fold=False``,
    three steps with a wrapping ring.  Bit-equality is not required (the one-pass head sums in another order, the clip's norm
    is an fp64 sum in another order) -- the tolerances are the fused step's own against its golden state
    (tests/test_train_step_emu.py)"""
    from gcc_amd.train_step import _GraphedStep

    monkeypatch.setattr(_GraphedStep, "RING_LEN", 2)
    sides = []
    for fold in (False, True):
        tr, model = _trainer(64)
        tr.fold, tr.onepass_head = fold, fold and onepass
        tr.use_scalars = True
        tr.dropout_seed = 0xABC
        outs = [tr.step(it, 0.005 * (1.0 - 0.2 * it)) for it in range(3)]
        sides.append(dict(loss=torch.stack([o["loss"] for o in outs]), prob=torch.stack([o["prob"] for o in outs]),
                          gnorm=tr.optimizer.grad_norm.clone(), flat=tr.flat.clone(), ema=tr.flat_ema.clone(),
                          grad=tr.flat_grad.clone(), mem=tr.contrast.memory.clone(), m=tr.optimizer.exp_avg.clone(),
                          count=int(tr.ring_counter)))
        assert tr.contrast.index == (3 * B) % 96
    a, b = sides
    assert a["count"] == b["count"] == 3
    for name in ("loss", "prob"):
        torch.testing.assert_close(a[name], b[name], rtol=1e-4, atol=1e-5, msg=lambda m, name=name: f"{name}: {m}")
    torch.testing.assert_close(a["gnorm"], b["gnorm"], rtol=1e-3, atol=1e-5)
    for name in ("mem", "m", "grad"):
        torch.testing.assert_close(a[name], b[name], rtol=1e-3, atol=2e-5, msg=lambda m, name=name: f"{name}: {m}")
    # The weights: Adam's update g / (|g| + 1e-8) is ill-conditioned where |g| ~ 1e-8 (an absolute change of 1e-9 in such an
    # element -- 1e-7 of the gradient's scale, what another summation order in the head moves it by -- turns the update by
    # percents of lr).  So: all but a vanishing share of the elements at the tolerance above, and none further apart than
    # three updates can carry it (|update| <= lr / (1 - beta1) at most, 3 steps).
    for name in ("flat", "ema"):
        d = (a[name] - b[name]).abs()
        off = d > 2e-5 + 1e-3 * b[name].abs()
        print(f"{name}: {int(off.sum())} of {d.numel()} elements outside rtol 1e-3 / atol 2e-5, largest difference {float(d.max()):.3e}")
        assert int(off.sum()) <= 1e-4 * d.numel() and float(d.max()) <= 3 * 0.005 / (1 - 0.9)
