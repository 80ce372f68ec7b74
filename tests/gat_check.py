"""Shared by the GAT tests: symmetric hand-built batches, encoders, and the comparison of the kernels' forward output and
every parameter gradient against the float64 restatement (tests/gat_reference.py)."""
import os

import numpy as np
import torch

from gcc_amd.encoder import GraphEncoder, gat_params
from tests.gat_reference import forward_of, params_of  # noqa: F401  (params_of: re-exported for the tests)


def gat_encoder(hidden=64, heads=4, layers=5, T=6, Lr=3, norm=True, pos=32, deg_emb=16, max_degree=512, seed=0, out=None):
    """``out``: output_dim (None: the hidden size)"""
    torch.manual_seed(seed)
    return GraphEncoder(positional_embedding_size=pos, max_node_freq=16, max_edge_freq=16, max_degree=max_degree,
                        freq_embedding_size=16, degree_embedding_size=deg_emb, output_dim=hidden if out is None else out,
                        node_hidden_dim=hidden,
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


def worst_rel_shared(got: dict, ref: dict):
    """:func:`worst_rel` with one change: the scale of ``gnn.layers.i.gnn.attn_r`` is the larger of its own float64 max-abs
    and that of ``gnn.layers.i.gnn.attn_l``.  Both gradients are the same kind of sum, sum over rows of d(logit) * ft,
    over the same rows and the same ft, so they share a rounding floor -- but the TRUE gradient of attn_r cancels to zero
    exactly whenever every logit into a node has the same sign (er_v is then a shift of all of v's logits, and a softmax
    ignores a shift), which deep layers reach.  Against its own max-abs of 1e-17 a float32 rounding residue of 3e-8 reads
    as a relative error of 1e9; against the floor it shares with attn_l it reads as what it is.  Every other tensor is
    scaled exactly as in worst_rel, so nothing else gets looser."""
    worst, name = 0.0, None
    for k, r in ref.items():
        scale = float(r.abs().max())
        if k.endswith(".gnn.attn_r"):
            scale = max(scale, float(ref[k[: -len("attn_r")] + "attn_l"].abs().max()))
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


# ---------------------------------------------------------------------------------------------------------------------
# The shape edges of csrc/gat.hip, shared by tests/test_gat_edges_emu.py and tests/test_gat_edges_gpu.py.
# A case: enc = gat_encoder arguments; sizes = node counts of the graphs; gen = symmetric_batch options; mult = edge
# multiplicity; seed_local = per-graph local index of the seed node (None: not passed); cap_extra = rows of capacity beyond
# the live nodes; repeat = every CSR entry appears twice in its row; poison = the padding rows of pos_undirected are NaN.
# No case has all-zero true gradients (hidden = 1, or output_dim = 1 with norm): no tolerance means anything against a
# zero scale.
_SMALL = dict(layers=2, T=2, Lr=1, pos=8, deg_emb=8, max_degree=16)


def _case(name, enc, sizes, gen=None, mult=1, seed_local=None, cap_extra=37, repeat=False, poison=False):
    return dict(name=name, enc={**_SMALL, **enc}, sizes=list(sizes), gen=dict(gen or {}), mult=mult, seed_local=seed_local,
                cap_extra=cap_extra, repeat=repeat, poison=poison)


EDGE_CASES = [
    # heads that do not divide 64: the backward walks a row in S = 64 / H edge slots per head; the hub rows are longer than S
    _case("h48_heads3_hub40", dict(hidden=48, heads=3), [6, 50, 3], dict(p=0.1, extra_star=(1, 40))),
    _case("h60_heads6_hub12", dict(hidden=60, heads=6), [9, 14], dict(extra_star=(1, 12))),
    _case("h40_heads5_hub15", dict(hidden=40, heads=5), [20, 5], dict(extra_star=(0, 15))),
    _case("h63_heads7_hub14", dict(hidden=63, heads=7), [7, 18], dict(extra_star=(1, 14))),
    _case("h64_heads1", dict(hidden=64, heads=1), [8, 5]),
    _case("h64_heads64", dict(hidden=64, heads=64), [8, 11]),
    # output_dim != hidden, both ways
    _case("h16_out64_norm", dict(hidden=16, heads=2, out=64, norm=True), [9, 4, 6]),
    _case("h16_out64_raw", dict(hidden=16, heads=2, out=64, norm=False), [9, 4, 6]),
    _case("h32_out7_norm", dict(hidden=32, heads=4, out=7, norm=True), [9, 4, 6]),
    _case("h32_out7_raw", dict(hidden=32, heads=4, out=7, norm=False), [9, 4, 6]),
    # depth and recurrence limits
    _case("T1_Lr1", dict(hidden=32, heads=4, T=1, Lr=1), [7, 5]),
    _case("T1_Lr3", dict(hidden=32, heads=4, T=1, Lr=3), [7, 5]),
    _case("L1", dict(hidden=32, heads=4, layers=1), [7, 5]),
    _case("L8_Lr8_h16", dict(hidden=16, heads=2, layers=8, Lr=8), [9, 6, 12]),
    _case("L8_h64", dict(hidden=64, heads=4, layers=8), [9, 6, 12]),
    # input width
    _case("pos0", dict(hidden=32, heads=4, pos=0), [7, 5], dict(pos_dim=0)),
    _case("K0_64", dict(hidden=32, heads=4, pos=47, deg_emb=16), [7, 5], dict(pos_dim=47)),
    _case("max_degree0", dict(hidden=32, heads=4, max_degree=0), [7, 5]),
    _case("mult3_max_degree4", dict(hidden=32, heads=4, max_degree=4), [8, 10], dict(p=0.5), mult=3),
    # batch shape
    _case("B1", dict(hidden=32, heads=4), [12]),
    _case("B70", dict(hidden=32, heads=4), [1 + i % 5 for i in range(70)]),
] + [
    _case(f"mid{n}", dict(hidden=32, heads=4), [5, n, 4], dict(p=min(0.3, 6.0 / n)), cap_extra=0)
    for n in (15, 16, 17, 63, 64, 65, 255, 256, 257, 1025)
] + [
    _case("seed_local", dict(hidden=32, heads=4), [6, 4, 9], seed_local=[3, 0, 5]),
    _case("repeated_entries", dict(hidden=32, heads=4), [8, 10], dict(p=0.4), repeat=True),
    _case("poisoned_padding", dict(hidden=32, heads=4), [9, 4, 6], poison=True),
    # edge-free batches: the CSR has no entry at all
    _case("edge_free_one_node", dict(hidden=32, heads=4), [1]),
    _case("edge_free_five_single_nodes", dict(hidden=32, heads=4), [1, 1, 1, 1, 1]),
    _case("edge_free_empty_graphs", dict(hidden=32, heads=4), [0, 0, 0]),
    _case("edge_free_mixed", dict(hidden=32, heads=4), [1, 0, 1]),
]
CASE_IDS = [c["name"] for c in EDGE_CASES]


def repeat_entries(batch):
    """every CSR entry twice in its row (what an edge list holding both directions of every edge twice becomes)"""
    out = dict(batch)
    out["row_ptr"] = batch["row_ptr"] * 2
    out["col_idx"] = batch["col_idx"].repeat_interleave(2)
    return out


def case_inputs(case):
    """-> (encoder, host batch dict, dout [B, out], keyword arguments of forward_of)"""
    enc = gat_encoder(**case["enc"])
    gen = dict(pos_dim=case["enc"]["pos"], seed=11)
    gen.update(case["gen"])
    batch = symmetric_batch(case["sizes"], **gen)
    if case["repeat"]:
        batch = repeat_entries(batch)
    dout = torch.randn(len(case["sizes"]), enc.output_dim, generator=torch.Generator().manual_seed(5))
    kw = dict(mult=case["mult"])
    if case["seed_local"] is not None:
        kw["seed_local"] = torch.tensor(case["seed_local"], dtype=torch.long)
    return enc, batch, dout, kw


def dress_batch(g, case):
    """the case's per-batch options on a batch object (CpuBatch or DeviceBatch)"""
    g.edge_multiplicity = case["mult"]
    if case["seed_local"] is not None:
        g.seed_local = torch.tensor(case["seed_local"], dtype=torch.int32, device=g.node_off.device)
    if case["poison"]:
        n = int(g.node_off[-1])
        assert g.pos_undirected.shape[0] > n, "a poisoned case needs padding rows"
        g.pos_undirected[n:] = float("nan")
    return g


class DeviceBatch:
    """A hand-built batch on ``device`` with ``cap_extra`` rows of capacity beyond the live nodes: the members that
    GatEngine reads of a BatchedCSR (graph_id's length is the capacity)."""

    def __init__(self, batch, cap_extra=37, device="cuda:0"):
        n = int(batch["node_off"][-1])
        cap = max(n + cap_extra, 1)
        self.batch_size = len(batch["node_off"]) - 1
        self.node_off = batch["node_off"].int().to(device)
        self.row_ptr = torch.cat([batch["row_ptr"], batch["row_ptr"][-1:].repeat(cap - n)]).int().to(device)
        self.col_idx = batch["col_idx"].int().to(device)
        self.graph_id = torch.zeros(cap, dtype=torch.int32, device=device)
        pos = batch["pos_undirected"]
        self.pos_undirected = torch.cat([pos, torch.zeros(cap - n, pos.shape[1])]).to(device)


def reference_of(enc, batch, dout, kw, dtype=torch.float64):
    """-> (out, {param name: grad}) of sum(out * dout) by the restatement in ``dtype``"""
    P = params_of(enc, dtype)
    out = forward_of(enc, P, batch, **kw)
    (out * dout.to("cpu", dtype)).sum().backward()
    # (a parameter that the output does not depend on -- the GAT layers of a batch of empty graphs -- has no .grad: zero)
    return out.detach(), {k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in P.items()}
