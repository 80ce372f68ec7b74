"""torch.autograd glue for the drop-in ``GraphEncoder.forward`` (API path).

The bench / train.py fast path (gcc_amd/train_step.py) drives the same C-ABI
calls directly and skips autograd.
"""
from __future__ import annotations

import torch

from ._cabi import raw_stream
from .encoder import STALE_SLOT_MSG, H, gat_params, grad_params


class _GinFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, g, keep, needs_backward, *params):
        eng = enc.engine()
        bn_training = enc.bn_training()
        p, buf = eng.make_pass(enc, g, training=bn_training, keep=keep, slot=enc.pass_slot(needs_backward))
        if not bn_training and getattr(enc, "fused_eval", True):
            eng.eval_fused([p], stream=raw_stream(g.node_off))     # eval mode: one launch, one workgroup per subgraph
        else:
            eng.forward([p], stream=raw_stream(g.node_off))
        ctx.enc, ctx.p, ctx.buf = enc, p, buf
        L = len(enc.gnn.ginlayers)
        outs = [buf["feat"].clone()] + [buf["pooled"][i + 1].float() for i in range(L)]
        ctx.mark_non_differentiable(*outs[1:])
        return tuple(outs)

    @staticmethod
    def backward(ctx, dfeat, *_unused):
        enc = ctx.enc
        if not ctx.p.training:
            raise RuntimeError("backward through an eval-mode (running statistics) pass is not supported")
        if not enc.engine().slot_is_current(ctx.buf):
            raise RuntimeError(STALE_SLOT_MSG)
        targets = [enc.padded_zeros_like(param) for _, _, param in grad_params(enc)]
        enc.engine().backward(enc, ctx.p, ctx.buf, dfeat, targets=targets, stream=raw_stream(dfeat))
        return (None, None, None, None, *targets)


def gin_apply(enc, g, return_all_outputs=False):
    """GraphEncoder.forward (graph_encoder.py:132-200) on a BatchedCSR."""
    keep = None
    if enc.gnn.drop.training and enc.gnn.drop.p > 0:          # gin.py:202,230 nn.Dropout(0.5)
        L = len(enc.gnn.ginlayers)
        keep = (torch.rand(L + 1, g.batch_size, H, device=g.node_off.device) >= enc.gnn.drop.p).float()
    params = [param for _, _, param in grad_params(enc)]
    outs = _GinFn.apply(enc, g, keep, enc.needs_backward(params), *params)
    x = outs[0]
    if return_all_outputs:
        return x, list(outs[1:])
    return x


class _GatFn(torch.autograd.Function):
    """GAT encoder + Set2Set + lin_readout + normalize (csrc/gat.hip).  The forward's activations are a tensor owned by
    this node (``ctx``), not an engine slot: any number of passes may be pending.  The parameters go through
    save_for_backward, so an in-place update between forward and backward (an optimizer step) raises, as in torch, instead
    of differentiating with the new weights the pass structs point at."""

    @staticmethod
    def forward(ctx, enc, g, *params):
        out, saved, p, w = enc.engine().forward(enc, g, stream=raw_stream(g.node_off))
        ctx.enc, ctx.g, ctx.p, ctx.w = enc, g, p, w
        ctx.saved_gat = saved          # p / w hold raw pointers into `saved` and the parameters of this pass
        ctx.save_for_backward(*params)
        return out

    @staticmethod
    def backward(ctx, dout):
        enc = ctx.enc
        params = ctx.saved_tensors     # (raises if a parameter was modified in place since the forward)
        targets = [torch.zeros_like(t) for t in params]
        enc.engine().backward(enc, ctx.p, ctx.w, dout, targets, stream=raw_stream(dout))
        return (None, None, *targets)


def gat_apply(enc, g):
    """GraphEncoder.forward for gnn_model="gat" (graph_encoder.py:132-196) on a BatchedCSR.  A pass nobody can
    differentiate (grad disabled, or no parameter requires grad) builds no autograd node; its `saved` buffer is released
    when the call returns."""
    params = [t for _, _, t in gat_params(enc)]
    if not (torch.is_grad_enabled() and any(t.requires_grad for t in params)):
        with torch.no_grad():
            out, _saved, _p, _w = enc.engine().forward(enc, g, stream=raw_stream(g.node_off))
        return out
    return _GatFn.apply(enc, g, *params)
