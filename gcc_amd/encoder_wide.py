"""GraphEncoder at hidden / output sizes above 64 (``--hidden-size``, train.py:93; graph_encoder.py:44-63): host side of
csrc/ginx.hip -- one C-ABI call for the forward pass (training or eval mode), one for the backward pass, plus the
autograd glue of the API path.  Same module tree, state_dict keys and arithmetic as the 64-channel path; what differs
is the kernels underneath (unfused, one launch per operator) and that dropout masks are drawn on the host side of the
call (torch.rand on the device, as torch.nn.Dropout draws them: gin.py:202,230).
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi
from ._cabi import raw_stream
from .encoder import STALE_SLOT_MSG, _fill_struct, fill_weights, grad_params


class WideGinEngine:
    """Workspaces + C-ABI calls of gcc_ginx_forward / gcc_ginx_backward.  ``lib`` / ``ptr`` are injectable only so that the
    tests can run the same host code against the emulator build."""

    def __init__(self, lib=None, ptr=None):
        self.lib = lib if lib is not None else _cabi.load()
        self.ptr = ptr if ptr is not None else _cabi.dev_ptr
        self._ws = {}
        self._gen = {}                      # workspace key -> generation: a forward stamps its slot, a backward checks the stamp

    def make_pass(self, enc, g, training, keep=None, slot=0, want_pooled=False):
        ptr = self.ptr
        L = len(enc.gnn.ginlayers)
        b = _cabi.bind_batch(g, ptr, need_graph_id=True)
        node_cap, B, dev = b.node_cap, b.batch_size, b.device
        d_in = enc.positional_embedding_size + enc.degree_embedding_size + 1
        nbytes = _cabi.size_query(self.lib, "gcc_ginx_workspace_bytes", node_cap, B, L, d_in, enc.hidden, enc.output_dim, named=False)
        key = (slot, nbytes, str(dev))
        if key not in self._ws:
            self._ws[key] = dict(ws=torch.zeros(nbytes, dtype=torch.uint8, device=dev),
                                 feat=torch.zeros(B, enc.output_dim, dtype=torch.float32, device=dev),
                                 pooled=torch.zeros(L, B, enc.hidden, dtype=torch.float32, device=dev))
        buf = self._ws[key]
        self._gen[key] = self._gen.get(key, 0) + 1
        p = _cabi.GccGinxPass(node_off=b.node_off, row_ptr=b.row_ptr, col_idx=b.col_idx, graph_id=b.graph_id, pos=b.pos,
                              seed_local=b.seed_local, batch_size=B, edge_multiplicity=b.edge_multiplicity, node_cap=node_cap)
        p.training, p.update_running_stats, p.normalize = int(training), int(training), int(enc.norm)
        p.dropout_keep = ptr(keep) if keep is not None else None
        p.hidden, p.out_dim = enc.hidden, enc.output_dim
        p.gemm_dtype = _cabi.GEMM_DTYPES[getattr(enc, "encoder_dtype", "f32")]      # (--encoder-dtype: the per-node Linears' operands)
        p.w = fill_weights(enc, ptr)
        p.workspace, p.workspace_bytes = ptr(buf["ws"]), nbytes
        p.feat = ptr(buf["feat"])
        p.pooled_out = ptr(buf["pooled"]) if want_pooled else None
        out = dict(buf)
        out["_keepalive"] = (g, keep, enc)          # the struct holds raw pointers into these
        out["_slot"] = (key, self._gen[key])        # which workspace this pass's activations live in, and its generation
        return p, out

    def forward(self, p, stream=None):
        _cabi.call(self.lib, "gcc_ginx_forward", ctypes.byref(p), stream)

    def slot_is_current(self, buf):
        """False once a later forward has reused the workspace slot this pass's activations were stored in."""
        key, gen = buf["_slot"]
        return self._gen.get(key) == gen

    def backward(self, enc, p, buf, dfeat, targets, stream=None):
        """Gradients of the pass ``(p, buf)`` of :meth:`make_pass` into ``targets`` (tensors in :func:`grad_params` order): the
        argument order of :meth:`GinEngine.backward` (the activations are addressed through ``p.workspace``)."""
        grads = _fill_struct(_cabi.GccGinGrads(), [(n, i, t) for (n, i, _), t in zip(grad_params(enc), targets)], self.ptr)
        dfeat = dfeat.contiguous()
        _cabi.call(self.lib, "gcc_ginx_backward", ctypes.byref(p), self.ptr(dfeat), ctypes.byref(grads), stream)
        return targets


class _GinxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, g, keep, want_pooled, needs_backward, *params):
        eng = enc.wide_engine()
        training = enc.bn_training()
        p, buf = eng.make_pass(enc, g, training=training, keep=keep, slot=enc.pass_slot(needs_backward), want_pooled=want_pooled)
        eng.forward(p, stream=raw_stream(g.node_off))
        ctx.enc, ctx.p, ctx.buf = enc, p, buf
        L = len(enc.gnn.ginlayers)
        outs = [buf["feat"].clone()] + ([buf["pooled"][i].clone() for i in range(L)] if want_pooled else [])
        ctx.mark_non_differentiable(*outs[1:])
        return tuple(outs)

    @staticmethod
    def backward(ctx, dfeat, *_unused):
        enc = ctx.enc
        if not ctx.p.training:
            raise RuntimeError("backward through an eval-mode (running statistics) pass is not supported")
        if not enc.wide_engine().slot_is_current(ctx.buf):
            raise RuntimeError(STALE_SLOT_MSG)
        targets = [torch.zeros_like(param) for _, _, param in grad_params(enc)]
        enc.wide_engine().backward(enc, ctx.p, ctx.buf, dfeat, targets, stream=raw_stream(dfeat))
        return (None, None, None, None, None, *targets)


def ginx_apply(enc, g, return_all_outputs=False):
    """GraphEncoder.forward (graph_encoder.py:132-200) on a BatchedCSR, any width."""
    keep = None
    if enc.gnn.drop.training and enc.gnn.drop.p > 0:          # gin.py:202,230 nn.Dropout(0.5)
        L = len(enc.gnn.ginlayers)
        keep = (torch.rand(L + 1, g.batch_size, enc.output_dim, device=g.node_off.device) >= enc.gnn.drop.p).float()
    params = [param for _, _, param in grad_params(enc)]
    outs = _GinxFn.apply(enc, g, keep, bool(return_all_outputs), enc.needs_backward(params), *params)
    if return_all_outputs:
        return outs[0], list(outs[1:])
    return outs[0]
