"""A float64 torch restatement of GraphEncoder(gnn_model="gat") (gat.py + graph_encoder.py:152-196 of the reference,
DGL 0.4.3's GATConv / edge softmax / Set2Set recalled): the yardstick of the GAT kernels.  Autograd gives its gradients.

Edges follow DGL's batched graph: CSR row u lists the targets v of the edges u -> v; attention is a softmax over the
incoming edges of v, and every CSR entry is one edge.  The in-degree counts ``mult`` (edge multiplicity).
"""
import torch
import torch.nn.functional as F


def params_of(enc, dtype=torch.float64):
    """name -> leaf tensor (requires_grad) in ``dtype`` for every parameter of a GAT GraphEncoder."""
    return {k: v.detach().to("cpu", dtype).clone().requires_grad_(True) for k, v in enc.named_parameters()}


def gat_forward(P, node_off, row_ptr, col_idx, pos, *, num_layers, heads, T, Lr, max_degree, norm=True, mult=1,
                seed_local=None, eps=1e-5):
    """P: dict of parameters by state_dict key; CSR arrays of ONE batch (live extents); -> [B, out]"""
    dt, dev = P["degree_embedding.weight"].dtype, P["degree_embedding.weight"].device
    node_off = torch.as_tensor(node_off, dtype=torch.long, device=dev)
    row_ptr = torch.as_tensor(row_ptr, dtype=torch.long, device=dev)
    n, B = int(node_off[-1]), len(node_off) - 1
    nnz = int(row_ptr[n])
    col_idx = torch.as_tensor(col_idx, dtype=torch.long, device=dev)[:nnz]
    src = torch.repeat_interleave(torch.arange(n, device=dev), row_ptr[1: n + 1] - row_ptr[:n])
    dst = col_idx
    gid = torch.repeat_interleave(torch.arange(B, device=dev), node_off[1:] - node_off[:-1])
    deg = torch.bincount(dst, minlength=n) * mult
    seed = torch.zeros(n, dtype=dt, device=dev)
    first = node_off[:-1] + (0 if seed_local is None else torch.as_tensor(seed_local, dtype=torch.long, device=dev))
    seed[first[node_off[1:] > node_off[:-1]]] = 1.0
    h = torch.cat((torch.as_tensor(pos)[:n].to(dev, dt), P["degree_embedding.weight"][deg.clamp(0, max_degree)], seed[:, None]), 1)
    for i in range(num_layers):
        pre = f"gnn.layers.{i}.gnn."
        W, al, ar = P[pre + "fc.weight"], P[pre + "attn_l"], P[pre + "attn_r"]
        D = W.shape[0]
        ft = (h @ W.t()).view(n, heads, D // heads)
        el, er = (ft * al).sum(-1), (ft * ar).sum(-1)                       # [n, H]
        e = F.leaky_relu(el[src] + er[dst], 0.2)                           # [E, H]
        emax = torch.full((n, heads), -torch.inf, dtype=dt, device=dev).index_reduce(0, dst, e.detach(), "amax")
        a = torch.exp(e - emax[dst])
        s = torch.zeros(n, heads, dtype=dt, device=dev).index_add(0, dst, a)
        a = a / s[dst]
        rst = torch.zeros(n, heads, D // heads, dtype=dt, device=dev).index_add(0, dst, a[..., None] * ft[src]).reshape(n, D)
        h = F.leaky_relu(rst) if i + 1 < num_layers else rst
    x = h
    D = x.shape[1]
    qstar = torch.zeros(B, 2 * D, dtype=dt, device=dev)
    hs = [torch.zeros(B, D, dtype=dt, device=dev) for _ in range(Lr)]
    cs = [torch.zeros(B, D, dtype=dt, device=dev) for _ in range(Lr)]
    for _ in range(T):
        inp = qstar
        for k in range(Lr):
            z = (inp @ P[f"set2set.lstm.weight_ih_l{k}"].t() + P[f"set2set.lstm.bias_ih_l{k}"]
                 + hs[k] @ P[f"set2set.lstm.weight_hh_l{k}"].t() + P[f"set2set.lstm.bias_hh_l{k}"])
            zi, zf, zg, zo = z.chunk(4, 1)
            cs[k] = torch.sigmoid(zf) * cs[k] + torch.sigmoid(zi) * torch.tanh(zg)
            hs[k] = torch.sigmoid(zo) * torch.tanh(cs[k])
            inp = hs[k]
        q = inp
        e = (x * q[gid]).sum(-1)
        if n:
            emax = torch.full((B,), -torch.inf, dtype=dt, device=dev).index_reduce(0, gid, e.detach(), "amax")
            a = torch.exp(e - emax[gid])
            a = a / torch.zeros(B, dtype=dt, device=dev).index_add(0, gid, a)[gid]
            r = torch.zeros(B, D, dtype=dt, device=dev).index_add(0, gid, a[:, None] * x)
        else:
            r = torch.zeros(B, D, dtype=dt, device=dev)
        qstar = torch.cat((q, r), 1)
    out = F.relu(qstar @ P["lin_readout.0.weight"].t() + P["lin_readout.0.bias"])
    out = out @ P["lin_readout.2.weight"].t() + P["lin_readout.2.bias"]
    if norm:
        out = F.normalize(out, p=2, dim=-1, eps=eps)
    return out


def forward_of(enc, P, batch, **kw):
    """gat_forward with the encoder's configuration; batch: dict node_off, row_ptr, col_idx, pos_undirected."""
    return gat_forward(P, batch["node_off"], batch["row_ptr"], batch["col_idx"], batch["pos_undirected"],
                       num_layers=len(enc.gnn.layers), heads=enc.num_heads, T=enc.num_step_set2set,
                       Lr=enc.set2set.lstm.num_layers, max_degree=enc.max_degree, norm=enc.norm, **kw)
