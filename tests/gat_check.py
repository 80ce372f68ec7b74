"""Shared by the GAT tests: symmetric hand-built batches, encoders, and the comparison of the kernels' forward output and
every parameter gradient against the float64 restatement (tests/gat_reference.py)."""
import os

import numpy as np
import torch

from gcc_amd.encoder import GraphEncoder, gat_params
from tests.gat_reference import forward_of, params_of  # noqa: F401  (params_of: re-exported for the tests)


def gat_encoder(hidden=64, heads=4, layers=5, T=6, Lr=3, norm=True, pos=32, deg_emb=16, max_degree=512, seed=0):
    torch.manual_seed(seed)
    return GraphEncoder(positional_embedding_size=pos, max_node_freq=16, max_edge_freq=16, max_degree=max_degree,
                        freq_embedding_size=16, degree_embedding_size=deg_emb, output_dim=hidden, node_hidden_dim=hidden,
                        edge_hidden_dim=hidden, num_layers=layers, num_heads=heads, num_step_set2set=T,
                        num_layer_set2set=Lr, norm=norm, gnn_model="gat", degree_input=True)


def symmetric_batch(sizes, p=0.3, pos_dim=32, seed=0, isolated=(), extra_star=None):
    """Random undirected graphs (CSR rows list neighbours, both directions) of the given node counts.
    ``isolated``: global node ids left without edges.  ``extra_star``: (graph index, leaves) adds a hub joined to
    ``leaves`` nodes of that graph (a long row)."""
    rng = np.random.default_rng(seed)
    node_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(node_off[-1])
    adj = [set() for _ in range(n)]
    for b, s in enumerate(sizes):
        o = node_off[b]
        for i in range(s):
            for j in range(i + 1, s):
                if rng.random() < p:
                    adj[o + i].add(o + j)
                    adj[o + j].add(o + i)
            if i > 0 and not adj[o + i]:                   # mostly connected
                j = int(rng.integers(0, i))
                adj[o + i].add(o + j)
                adj[o + j].add(o + i)
    if extra_star is not None:
        b, leaves = extra_star
        o, s = node_off[b], sizes[b]
        for j in range(1, min(leaves + 1, s)):
            adj[o].add(o + j)
            adj[o + j].add(o)
    for v in isolated:
        for u in adj[v]:
            adj[u].discard(v)
        adj[v] = set()
    row_ptr = np.zeros(n + 1, np.int64)
    cols = []
    for v in range(n):
        nb = sorted(adj[v])
        cols += nb
        row_ptr[v + 1] = row_ptr[v] + len(nb)
    pos = torch.from_numpy(rng.standard_normal((n, pos_dim))).float()
    return dict(node_off=torch.from_numpy(node_off), row_ptr=torch.from_numpy(row_ptr),
                col_idx=torch.tensor(cols, dtype=torch.long), pos_undirected=pos)


def reference(enc, batch, dout, mult=1):
    """-> (out float64, {param name: grad float64}) of sum(out * dout)."""
    P = params_of(enc)
    out = forward_of(enc, P, batch, mult=mult)
    (out * dout.double()).sum().backward()
    return out.detach(), {k: v.grad for k, v in P.items()}


def kernel_grads(enc, engine, g, dout, stream=None):
    """forward + backward through the engine -> (out, {param name: grad})"""
    out, saved, p, w = engine.forward(enc, g, stream=stream)
    targets = [torch.zeros_like(t) for _, _, t in gat_params(enc)]
    engine.backward(enc, p, w, dout, targets, stream=stream)
    names = {id(t): k for k, t in enc.named_parameters()}
    return out, {names[id(t)]: gt for (_, _, t), gt in zip(gat_params(enc), targets)}, saved


def worst_rel(got: dict, ref: dict):
    """max over tensors of max|got - ref| / max|ref| -> (value, tensor name)"""
    worst, name = 0.0, None
    for k, r in ref.items():
        scale = float(r.abs().max())
        err = float((got[k].double().cpu() - r).abs().max())
        rel = err / scale if scale > 0 else err
        if rel > worst:
            worst, name = rel, k
    return worst, name


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gat_golden.pt")


def load_golden():
    return torch.load(GOLDEN, map_location="cpu", weights_only=False)


def moco_loss(feat_q, feat_k, memory, T):
    """MemoryMoCo.forward (use_softmax) + NCESoftmaxLoss of the reference, in the inputs' dtype"""
    l_pos = (feat_q * feat_k.detach()).sum(1, keepdim=True)
    l_neg = feat_q @ memory.detach().t()
    out = torch.cat((l_pos, l_neg), 1) / T
    return torch.nn.functional.cross_entropy(out, torch.zeros(out.shape[0], dtype=torch.long, device=out.device))


def golden_encoder(gold):
    enc = GraphEncoder(**gold["cfg"])
    enc.load_state_dict(gold["init"], strict=True)
    return enc


def check_golden_step(enc, step, gold, run, tol=1e-4):
    """run(enc, batch, mult, dout or None) -> (feat, {name: grad} or None): the kernels' forward (and backward of dout)
    on one view.  Checks feat_q, feat_k, the loss and every gradient against the reference's recorded ones."""
    mult = step["edge_multiplicity"]
    feat_k, _ = run(enc, step["k"], mult, None)
    feat_q, _ = run(enc, step["q"], mult, None)
    fq = feat_q.detach().cpu().double().requires_grad_(True)
    loss = moco_loss(fq, feat_k.detach().cpu().double(), step["memory"].double(), gold["nce_t"])
    loss.backward()
    _, grads = run(enc, step["q"], mult, fq.grad.float())
    torch.testing.assert_close(feat_q.cpu(), step["feat_q"], rtol=tol, atol=tol)
    torch.testing.assert_close(feat_k.cpu(), step["feat_k"], rtol=tol, atol=tol)
    torch.testing.assert_close(loss.float(), step["loss"], rtol=tol, atol=tol)
    worst, name = worst_rel(grads, {k: v.double() for k, v in step["grads"].items()})
    assert worst < 10 * tol, (worst, name)
