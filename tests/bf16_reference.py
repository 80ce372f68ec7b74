"""The bf16-operand rule of csrc/ginx.hip's ginx_gemm_bf16_kernel (gcc_ginx_pass.gemm_dtype = 1, gcc_ncex_forward_dt), restated
with plain torch -- TEST INFRASTRUCTURE ONLY.

    C = alpha * sum_k bf16(A(m, k)) * bf16(B(k, n)) [+ bias]

bf16() = round to nearest even (``tensor.bfloat16()``), products and sums in a wider type.  A bf16 x bf16 product has 16
significant bits and is exact in fp32, so once the operands are rounded only the order of the summation is left to an
implementation: the same model run in float64 ON THE ROUNDED VALUES is the exact value of the rule.

* :class:`RoundedLinearFn` / :class:`RoundedLinear`: a Linear whose forward, data gradient and weight gradient follow the rule
  (the bias gradient is a plain column sum); :func:`round_gin_linears` swaps it into the GIN layers' MLPs of an
  ``oracle.encoder.OracleGraphEncoder`` -- the [B, .] readout Linears (``linears_prediction``) stay plain.
* :func:`moco_head` / :func:`e2e_head`: the dense head's three products (logits, d loss / d rows, d loss / d mem) under the rule,
  everything else (positive logit, softmax, cross entropy) plain.
"""
import torch
import torch.nn.functional as F
from torch import nn


def r(t):
    """fp32 -> bf16 -> back, round to nearest even; a float64 tensor is rounded from its fp32 value and comes back float64."""
    return t.float().bfloat16().to(t.dtype)


class RoundedLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        return F.linear(r(x), r(W)) + b

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        return r(dy) @ r(W), r(dy).t() @ r(x), dy.sum(0)


class RoundedLinear(nn.Module):
    """Shares ``weight`` / ``bias`` (the Parameter objects, so names and .grad stay where they were) with the Linear it replaces."""

    def __init__(self, lin):
        super().__init__()
        self.weight, self.bias = lin.weight, lin.bias

    def forward(self, x):
        return RoundedLinearFn.apply(x, self.weight, self.bias)


def round_gin_linears(oracle):
    """In place: ginlayers[*].apply_func.mlp.linears[0 / 1] -> RoundedLinear.  Returns the model."""
    for layer in oracle.gnn.ginlayers:
        mlp = layer.apply_func.mlp
        for j in range(len(mlp.linears)):
            if not isinstance(mlp.linears[j], RoundedLinear):
                mlp.linears[j] = RoundedLinear(mlp.linears[j])
    return oracle


def _ce(out, labels):
    lse = torch.logsumexp(out, dim=1)
    picked = out.gather(1, labels.view(-1, 1)).squeeze(1)
    dlog = torch.softmax(out, dim=1)
    dlog[torch.arange(out.shape[0]), labels] -= 1.0
    return (lse - picked).mean(), picked.mean(), dlog


def moco_head(q, k, mem, T):
    """mode 0 of gcc_ncex_forward_dt(gemm_dtype = 1) in the dtype of its arguments (pass float64 for the exact value):
    -> dict(out [B, K + 1], loss, prob, grad_q) for a unit upstream gradient, against ``mem`` as it is."""
    B = q.shape[0]
    out = torch.cat(((q * k).sum(1, keepdim=True), r(q) @ r(mem).t()), dim=1) / T
    loss, prob, dlog = _ce(out, torch.zeros(B, dtype=torch.long))
    grad_q = (r(dlog[:, 1:]) @ r(mem) + dlog[:, :1] * k) / (T * B)
    return dict(out=out, loss=loss, prob=prob, grad_q=grad_q)


def e2e_head(fq, fk, T):
    """mode 1 (rows = feat_k, columns = feat_q, labels on the diagonal: train.py:400, criterions.py:27-33)
    -> dict(out [B, B], loss, prob, grad_q, grad_k)."""
    B = fq.shape[0]
    out = r(fk) @ r(fq).t() / T
    loss, prob, dlog = _ce(out, torch.arange(B))
    return dict(out=out, loss=loss, prob=prob, grad_k=r(dlog) @ r(fq) / (T * B), grad_q=r(dlog).t() @ r(fk) / (T * B))
