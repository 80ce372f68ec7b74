"""Test-side reference of gcc_ginw_embed (GraphEncoder.resident_eval): the feature rows in numpy, the layers through
oracle/gin_wide.py (fold_layer / gin_wide_forward), the readout in float64.  TEST INFRASTRUCTURE ONLY.

Two evaluations of the same model on the same batch:
  bf16=True   the rounding rule of DESIGN.md section 7b: feature rows and weights rounded to bf16, agg / z1 / h rounded where
              the kernel stores them, everything else float64 -- what the kernel is held to at 1e-3 per graph;
  bf16=False  nothing rounded, float64 throughout: the truth, which the kernel is held to at 2e-2 per graph.
"""
import numpy as np
import torch

from oracle import gin_wide as ow

D = 256


def ego_views(rng, sizes, pos_dim=32, hub=0.8, extra=1.0):
    """One view of a batch of ego-nets: node 0 of every subgraph is a hub adjacent to about ``hub`` of the others, plus about
    ``extra`` random edges per node; simple and symmetric; a subgraph of one node has no edge.  -> the dict CpuBatch takes."""
    node_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = []
    for b, n in enumerate(sizes):
        adj = np.zeros((n, n), dtype=bool)
        if n > 1:
            adj[0, 1:] = rng.random(n - 1) < hub
            adj[0, 1] = True
            for _ in range(int(extra * n)):
                u, v = rng.integers(0, n, 2)
                if u != v:
                    adj[u, v] = True
            adj = adj | adj.T
        rows += [np.nonzero(adj[v])[0] + node_off[b] for v in range(n)]
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col_idx = np.concatenate(rows).astype(np.int64)
    pos = rng.standard_normal((int(node_off[-1]), pos_dim)).astype(np.float32)
    pos /= np.linalg.norm(pos, axis=1, keepdims=True)
    return dict(node_off=torch.from_numpy(node_off), row_ptr=torch.from_numpy(row_ptr), col_idx=torch.from_numpy(col_idx),
                pos_undirected=torch.from_numpy(pos))


def randomize_running_stats(enc, seed):
    """eval-mode BatchNorm with non-trivial statistics and affine parameters, so that the fold is exercised"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(torch.rand(m.running_mean.shape, generator=g) - 0.5)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) * 0.6 - 0.2)


def feature_rows(enc, g, mult):
    """graph_encoder.py:152-165 for the live rows of batch ``g``: positional embedding | degree embedding | seed flag
    -> float32 [N, d_in].  In-degree = row length x edge multiplicity, clamped to max_degree; seed = seed_local or node 0."""
    node_off = g.node_off.cpu().numpy().astype(np.int64)
    n = int(node_off[-1])
    row_ptr = g.row_ptr.cpu().numpy().astype(np.int64)[: n + 1]
    deg = np.clip(np.diff(row_ptr) * mult, 0, enc.max_degree)
    emb = enc.degree_embedding.weight.detach().cpu().numpy()
    seed_local = getattr(g, "seed_local", None)
    seeds = node_off[:-1] + (seed_local.cpu().numpy().astype(np.int64) if seed_local is not None else 0)
    flag = np.zeros((n, 1), dtype=np.float32)
    flag[seeds[np.diff(node_off) > 0]] = 1.0
    return np.concatenate([g.pos_undirected.cpu().numpy()[:n].astype(np.float32), emb[deg], flag], axis=1)


def folded_layers(enc):
    """oracle/gin_wide.fold_layer on the encoder's modules, zero-padded to 256 channels"""
    def bn(m):
        return tuple(t.detach().cpu().numpy() for t in (m.weight, m.bias, m.running_mean, m.running_var))

    layers = []
    for i, layer in enumerate(enc.gnn.ginlayers):
        mlp = layer.apply_func.mlp
        ly = ow.fold_layer(mlp.linears[0].weight.detach().cpu().numpy(), mlp.linears[0].bias.detach().cpu().numpy(), bn(mlp.batch_norms[0]),
                           mlp.linears[1].weight.detach().cpu().numpy(), mlp.linears[1].bias.detach().cpu().numpy(), bn(layer.apply_func.bn),
                           bn(enc.gnn.batch_norms[i]), eps=mlp.batch_norms[0].eps)
        out = {}
        for k, v in ly.items():
            pad = np.zeros((D, D) if v.ndim == 2 else (D,), dtype=np.float32)
            pad[tuple(slice(0, s) for s in v.shape)] = v
            out[k] = pad
        layers.append(out)
    return layers


def view_pooled(enc, g, mult, bf16):
    """-> pooled [B, L + 1, 256] of one view on the multigraph (every CSR entry ``mult`` times)"""
    node_off = g.node_off.cpu().numpy().astype(np.int64)
    n = int(node_off[-1])
    row_ptr = g.row_ptr.cpu().numpy().astype(np.int64)[: n + 1]
    col_idx = g.col_idx.cpu().numpy().astype(np.int64)[: row_ptr[-1]]
    x = np.zeros((n, D), dtype=np.float32)
    f = feature_rows(enc, g, mult)
    x[:, : f.shape[1]] = ow.bf16_round(f) if bf16 else f
    _, pooled = ow.gin_wide_forward(node_off, row_ptr * mult, np.repeat(col_idx, mult), x, folded_layers(enc), bf16=bf16)
    return pooled


def readout(enc, pooled):
    """gin.py:226-230 in eval mode + graph_encoder.py:195-196, float64.  pooled [B, L + 1, 256] -> [B, output_dim]"""
    d_in = enc.positional_embedding_size + enc.degree_embedding_size + 1
    score = 0.0
    for i, lin in enumerate(enc.gnn.linears_prediction):
        k = d_in if i == 0 else enc.hidden
        score = score + pooled[:, i, :k].astype(np.float64) @ lin.weight.detach().cpu().numpy().astype(np.float64).T \
            + lin.bias.detach().cpu().numpy().astype(np.float64)
    if enc.norm:
        score = score / np.maximum(np.linalg.norm(score, axis=1, keepdims=True), 1e-5)
    return score


def reference_embedding(enc, views, mult, bf16=True):
    """(f(q) + f(k)) / 2, or f(q) for one view (generate.py:45-52) -> float64 [B, output_dim]"""
    fs = [readout(enc, view_pooled(enc, g, mult, bf16)) for g in views]
    return fs[0] if len(fs) == 1 else (fs[0] + fs[1]) / 2


def graph_errors(got, want):
    """relative Frobenius distance of every graph's embedding"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.linalg.norm(got - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-30)


BAR_RULE = 1e-3      # against the bf16-rule reference (tests/test_gin_wide_emu.py's bar for the pooled sums)
BAR_TRUTH = 2e-2     # against float64 without rounding (that file's bar against the truth)


def check_bars(got, enc, views, mult, label=""):
    """prints both figures per graph, then asserts both bars"""
    e_rule = graph_errors(got, reference_embedding(enc, views, mult, bf16=True))
    e_truth = graph_errors(got, reference_embedding(enc, views, mult, bf16=False))
    print(f"{label} per-graph error vs the bf16 rule: " + " ".join(f"{e:.1e}" for e in e_rule))
    print(f"{label} per-graph error vs the truth:     " + " ".join(f"{e:.1e}" for e in e_truth))
    assert (e_rule < BAR_RULE).all(), (label, e_rule)
    assert (e_truth < BAR_TRUTH).all(), (label, e_truth)
    return e_rule, e_truth
