"""Generates tests/golden/gat_golden.pt by EXECUTING THE REFERENCE'S OWN CODE (/root/reference/gcc/models/{gat,
graph_encoder}.py, gcc/contrastive/{memory_moco,criterions}.py) on CPU, with DGL replaced by tests/golden/dgl_stub.py
plus the DGL 0.4.3 pieces the GAT path calls, restated below ("DGL-recalled", as in dgl_stub.py):

  GATConv        fc (no bias) -> [N, H, F]; el / er = sum_f ft * attn_l / attn_r; e = leaky_relu(el_u + er_v, 0.2) on
                 every edge u -> v; edge_softmax over each node's incoming edges; rst_v = sum_u a_uv ft_u;
                 reset_parameters: xavier_normal_(gain=calculate_gain("relu")) on fc.weight, attn_l, attn_r
  GATLayer       (dgl.model_zoo.chem.gnn) GATConv, flatten over heads, then the activation
  Set2Set        LSTM(2d, d, n_layers), reset_parameters() called by __init__; forward: q, (h, c) = lstm(q*, (h, c)),
                 e = <x, q_b>, softmax over the graph's nodes, r_b = sum alpha x, q* = [q, r]

/root/reference does not exist on the GPU box, so the vectors are committed.  Run from the repo root:

    python tests/golden/make_gat_golden.py

Contents: a GAT GraphEncoder (hidden 64, 4 heads, 3 layers, Set2Set 3 x 1) and its EMA copy; the initial state_dict
under torch.manual_seed(SEED); two MoCo steps (train.py:388-407) without an optimizer step between them: inputs (the
second batch has an empty and a one-node graph; the first is a multigraph whose every edge is doubled -- recorded as the
simple CSR plus edge_multiplicity 2), the queue before each step, feat_q, feat_k, the loss and every parameter gradient.
"""
import copy
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import dgl_stub  # noqa: E402

SEED = 7
CFG = dict(positional_embedding_size=16, max_node_freq=16, max_edge_freq=16, max_degree=32, freq_embedding_size=16,
           degree_embedding_size=16, output_dim=64, node_hidden_dim=64, edge_hidden_dim=64, num_layers=3, num_heads=4,
           num_step_set2set=3, num_layer_set2set=1, norm=True, gnn_model="gat", degree_input=True)
K, NCE_T = 32, 0.07


class Graph(dgl_stub.StubBatchedGraph):
    """the stub's batched graph; the seed flag only for non-empty graphs (empty padding graphs have none)"""

    def __init__(self, node_off, row_ptr, col_idx, pos_undirected):
        super().__init__(node_off, row_ptr, col_idx, pos_undirected)
        seed = torch.zeros(self.number_of_nodes(), dtype=torch.long)
        live = self.node_off[1:] > self.node_off[:-1]
        seed[self.node_off[:-1][live]] = 1
        self.ndata["seed"] = seed


def edge_softmax(graph, e):                                   # [E, H] -> softmax over the incoming edges of each node
    n = graph.number_of_nodes()
    emax = torch.full((n,) + e.shape[1:], -torch.inf).index_reduce(0, graph.dst, e.detach(), "amax")
    a = torch.exp(e - emax[graph.dst])
    return a / torch.zeros((n,) + e.shape[1:]).index_add(0, graph.dst, a)[graph.dst]


class GATConv(nn.Module):
    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2, residual=False,
                 activation=None):
        super().__init__()
        self._num_heads, self._in_feats, self._out_feats = num_heads, in_feats, out_feats
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.FloatTensor(size=(1, num_heads, out_feats)))
        self.attn_r = nn.Parameter(torch.FloatTensor(size=(1, num_heads, out_feats)))
        self.feat_drop = nn.Dropout(feat_drop)
        self.attn_drop = nn.Dropout(attn_drop)
        self.leaky_relu = nn.LeakyReLU(negative_slope)
        assert not residual
        self.register_buffer("res_fc", None)
        self.reset_parameters()
        self.activation = activation

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)

    def forward(self, graph, feat):
        ft = self.fc(self.feat_drop(feat)).view(-1, self._num_heads, self._out_feats)
        el = (ft * self.attn_l).sum(dim=-1).unsqueeze(-1)
        er = (ft * self.attn_r).sum(dim=-1).unsqueeze(-1)
        e = self.leaky_relu(el[graph.src] + er[graph.dst])                         # apply_edges(u_add_v)
        a = self.attn_drop(edge_softmax(graph, e))
        rst = torch.zeros_like(ft).index_add(0, graph.dst, ft[graph.src] * a)     # update_all(u_mul_e, sum)
        if self.activation:
            rst = self.activation(rst)
        return rst


class GATLayer(nn.Module):
    def __init__(self, in_feats, out_feats, num_heads, feat_drop, attn_drop, alpha=0.2, residual=True, agg_mode="flatten",
                 activation=None):
        super().__init__()
        self.gnn = GATConv(in_feats=in_feats, out_feats=out_feats, num_heads=num_heads, feat_drop=feat_drop,
                           attn_drop=attn_drop, negative_slope=alpha, residual=residual)
        assert agg_mode in ["flatten", "mean"]
        self.agg_mode = agg_mode
        self.activation = activation

    def forward(self, bg, feats):
        new_feats = self.gnn(bg, feats)
        new_feats = new_feats.flatten(1) if self.agg_mode == "flatten" else new_feats.mean(1)
        if self.activation is not None:
            new_feats = self.activation(new_feats)
        return new_feats


class Set2Set(nn.Module):
    def __init__(self, input_dim, n_iters, n_layers):
        super().__init__()
        self.input_dim, self.output_dim = input_dim, 2 * input_dim
        self.n_iters, self.n_layers = n_iters, n_layers
        self.lstm = nn.LSTM(self.output_dim, self.input_dim, n_layers)
        self.reset_parameters()

    def reset_parameters(self):
        self.lstm.reset_parameters()

    def forward(self, graph, feat):
        B = graph.batch_size
        h = (feat.new_zeros((self.n_layers, B, self.input_dim)), feat.new_zeros((self.n_layers, B, self.input_dim)))
        q_star = feat.new_zeros(B, self.output_dim)
        gid = graph.graph_id
        for _ in range(self.n_iters):
            q, h = self.lstm(q_star.unsqueeze(0), h)
            q = q.view(B, self.input_dim)
            e = (feat * q[gid]).sum(dim=-1, keepdim=True)                             # broadcast_nodes
            emax = torch.full((B, 1), -torch.inf).index_reduce(0, gid, e.detach(), "amax")
            alpha = torch.exp(e - emax[gid])                                           # softmax_nodes
            alpha = alpha / torch.zeros(B, 1).index_add(0, gid, alpha)[gid]
            readout = torch.zeros(B, self.input_dim).index_add(0, gid, feat * alpha)   # sum_nodes (0 for an empty graph)
            q_star = torch.cat([q, readout], dim=-1)
        return q_star


from tests.gat_check import symmetric_batch  # noqa: E402  (before /root/reference, whose own tests/ would shadow it)

dgl_stub.install()
sys.modules["dgl.model_zoo.chem.gnn"].GATLayer = GATLayer
sys.modules["dgl.nn.pytorch"].Set2Set = Set2Set
sys.path.insert(0, "/root/reference")
torch.Tensor.cuda = lambda self, *a, **k: self          # memory_moco.py:56, criterions.py:15 call .cuda()

from gcc.contrastive.criterions import NCESoftmaxLoss  # noqa: E402
from gcc.contrastive.memory_moco import MemoryMoCo  # noqa: E402
from gcc.models import GraphEncoder  # noqa: E402


def doubled(batch):
    """the multigraph of a simple CSR whose every edge appears twice"""
    rp, ci = batch["row_ptr"], batch["col_idx"]
    n = len(rp) - 1
    cols = torch.cat([torch.cat([ci[rp[v]:rp[v + 1]], ci[rp[v]:rp[v + 1]]]) for v in range(n)]) if n else ci
    return dict(batch, row_ptr=2 * rp, col_idx=cols)


def main():
    P = CFG["positional_embedding_size"]
    views = [  # (q, k, edge multiplicity)
        (symmetric_batch([7, 11, 5, 9], pos_dim=P, p=0.3, seed=11), symmetric_batch([6, 12, 4, 10], pos_dim=P, p=0.3, seed=12), 2),
        (symmetric_batch([8, 0, 1, 13, 6], pos_dim=P, p=0.25, seed=13),
         symmetric_batch([9, 0, 1, 12, 7], pos_dim=P, p=0.25, seed=14), 1),
    ]
    torch.manual_seed(SEED)
    model = GraphEncoder(**CFG)
    model_ema = copy.deepcopy(model)
    init = {k: v.clone() for k, v in model.state_dict().items()}
    contrast = MemoryMoCo(CFG["output_dim"], None, K, NCE_T, use_softmax=True)
    criterion = NCESoftmaxLoss()
    model.train()
    model_ema.eval()
    steps = []
    for q, k, mult in views:
        ref_q, ref_k = (doubled(q), doubled(k)) if mult == 2 else (q, k)
        gq = Graph(ref_q["node_off"], ref_q["row_ptr"], ref_q["col_idx"], ref_q["pos_undirected"])
        gk = Graph(ref_k["node_off"], ref_k["row_ptr"], ref_k["col_idx"], ref_k["pos_undirected"])
        memory = contrast.memory.clone()
        model.zero_grad()
        feat_q = model(gq)
        with torch.no_grad():
            feat_k = model_ema(gk)
        out = contrast(feat_q, feat_k)
        loss = criterion(out)
        loss.backward()
        steps.append(dict(q=q, k=k, edge_multiplicity=mult, memory=memory, feat_q=feat_q.detach().clone(),
                          feat_k=feat_k.detach().clone(), loss=loss.detach().clone(),
                          grads={n: p.grad.clone() for n, p in model.named_parameters()}))
    gold = dict(cfg=CFG, seed=SEED, nce_k=K, nce_t=NCE_T, init=init, steps=steps)
    path = os.path.join(HERE, "gat_golden.pt")
    torch.save(gold, path)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; losses {[float(s['loss']) for s in steps]}")


if __name__ == "__main__":
    main()
