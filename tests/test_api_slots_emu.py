"""Workspace slots of the API path (GraphEncoder.forward under autograd): the activations of a forward that is pending a
backward live in one of two slots per encoder (model(q), model(k) of an E2E step).  A pass that cannot be backpropagated --
under torch.no_grad(), or in eval mode -- must not overwrite them, and a third grad-enabled forward must make the stale
backward raise instead of returning gradients computed from another batch's activations.  Both engines: the fused
64-channel kernels (width 64) and csrc/ginx.hip (width 128).  Emulator tier."""
import copy

import pytest
import torch

from tests.hipemu.emu_encoder import emu_engine
from tests.test_wide_encoder_emu import emu_wide_engine, fixed_views, wide_encoder

LAYERS = 3


def _model(width):
    torch.manual_seed(width)
    model = wide_encoder(width, width, LAYERS)
    assert model.wide == (width > 64)
    if model.wide:
        model._wide_engine = emu_wide_engine()
    else:
        model._engine = emu_engine()
    model.train()
    return model


def _views():
    q, k = fixed_views()
    r = copy.copy(q)                     # q's structure and node_cap (the same buffers), another positional embedding
    r.pos_undirected = torch.nn.functional.normalize(torch.randn(q.pos_undirected.shape, generator=torch.Generator().manual_seed(13)), dim=1)
    return q, k, r


def _keep(width, B):
    return (torch.rand(LAYERS, B, width, generator=torch.Generator().manual_seed(width + 1)) >= 0.5).float()


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("width", [64, 128])
def test_a_pass_without_backward_leaves_the_pending_backwards_alone(width, monkeypatch):
    q, k, r = _views()
    keep = _keep(width, q.batch_size)
    monkeypatch.setattr(torch, "rand", lambda *a, **kw: keep.clone())       # the API path draws its dropout masks here
    dq = torch.randn(q.batch_size, width, generator=torch.Generator().manual_seed(3))
    dk = torch.randn(q.batch_size, width, generator=torch.Generator().manual_seed(4))

    def run(third):
        model = _model(width)
        fq, fk = model(q), model(k)
        if third == "no_grad":
            with torch.no_grad():
                fr = model(r)
        elif third == "eval":
            model.eval()
            fr = model(r)
            model.train()
        fq.backward(dq)
        gq = _grads(model)
        model.zero_grad()
        fk.backward(dk)
        return gq, _grads(model), (fr.detach().clone() if third else None)

    base_q, base_k, _ = run(None)
    assert base_q and base_k
    for third in ("no_grad", "eval"):
        gq, gk, fr = run(third)
        assert torch.isfinite(fr).all()
        for name, g in base_q.items():
            assert torch.equal(gq[name], g), f"{third}: d {name} of model(q) changed after a third pass"
        for name, g in base_k.items():
            assert torch.equal(gk[name], g), f"{third}: d {name} of model(k) changed after a third pass"


@pytest.mark.parametrize("width", [64, 128])
def test_a_third_pending_forward_makes_the_overwritten_backward_raise(width, monkeypatch):
    q, k, r = _views()
    keep = _keep(width, q.batch_size)
    monkeypatch.setattr(torch, "rand", lambda *a, **kw: keep.clone())
    model = _model(width)
    fq, fk, fr = model(q), model(k), model(r)            # fr takes fq's slot
    with pytest.raises(RuntimeError, match="activations were overwritten"):
        fq.sum().backward()
    fk.sum().backward()                                   # the two passes still in their slots backpropagate
    fr.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
