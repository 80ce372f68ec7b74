"""Shared by tests/test_gin_edges_emu.py and tests/test_gin_edges_gpu.py: the fused 64-channel GIN pass (csrc/encoder.hip,
encoder_bwd.hip, encoder_common.h), ONE training-mode forward and backward per case against oracle/encoder.py in float64, at the
shapes where the tile kernels, the readout and the degree-embedding gradient change path.  TEST INFRASTRUCTURE ONLY.

Inputs and models are generated on the CPU from fixed seeds and then moved (tests/wide_edges_check.py::Tier), so the emulator
tier and the device tier run the same numbers.

Bars: none are chosen here.  ``feat`` at tests/test_encoder_gpu.py::TOL (rtol 1e-4 / atol 2e-5), BatchNorm running statistics at
that file's rtol 1e-4 / atol 1e-5, every gradient at tests/wide_step_check.py::grad_bar (1e-3 of the tensor's largest entry
against float64).  Every case also asserts the REFERENCE condition: torch's fp32 run of the oracle is inside the same gradient
bar against float64; a case that fails it is a wrong input ("BAD INPUT") and gets another seed or graph, never another bar.

Three input conditions, all asserted on the inputs or on the reference (build_graphs, build_models, reference): every BatchNorm
affine is randomised -- with weight 1 / bias 0 the gradients of apply_func.bn.weight and batch_norms.*.weight are structurally zero
(the next BatchNorm is scale invariant) and both sides hold noise only; no graph is complete -- on a complete graph every node
aggregates the same features, and with one graph in the batch the BatchNorm variance is rounding noise; and no float64
pre-activation lies within 2e-5 (the forward bar's absolute tolerance) of a ReLU kink, where any two fp32 implementations may
disagree on the element's mask.  The cases' seeds were searched with the ORACLE alone (the first of seed, seed + 100, ... that meets
the conditions); no kernel result entered the choice.

Worst figures over the 25 cases (the kernels | torch's fp32 run of the oracle, each against float64; torch's own figures move a
little with the host's thread count):
    emulator build:  feat 1.2e-6 | 2.2e-6 absolute; gradients 7.9e-5 | 1.6e-4 of the tensor's largest entry (bar 1e-3)
    MI355X:          feat 9.3e-7 | 2.2e-6 absolute; gradients 4.0e-5 | 1.5e-4 of the tensor's largest entry (bar 1e-3)
The per-case figures of the device run are in tests/test_gin_edges_gpu.py."""
import copy

import numpy as np
import torch

from gcc_amd.encoder import GraphEncoder
from oracle import encoder as E
from tests.hipemu.emu_encoder import CpuBatch
from tests.test_encoder_gpu import TOL
from tests.wide_step_check import grad_bar

H = 64
TILE = 64                # kTile of csrc/encoder_common.h
EMB_LDS_FLOATS = 10240   # kEmbMaxElems of csrc/encoder_bwd.hip
STAT_TOL = dict(rtol=1e-4, atol=1e-5)


def case(sizes, seed, *, node_cap=None, rows_hint=None, layers=5, pos=32, emb=16, max_degree=512, strip=(), star=False,
         seed_local=None, accumulate=False, expect=None):
    return dict(sizes=list(sizes), seed=seed, node_cap=node_cap, rows_hint=rows_hint, layers=layers, pos=pos, emb=emb,
                max_degree=max_degree, strip=tuple(strip), star=star, seed_local=seed_local, accumulate=accumulate,
                expect=expect or (lambda c, g, deg: None))


def _small(n, seed):
    """n graphs of 3..9 nodes"""
    return [int(s) for s in np.random.default_rng(seed).integers(3, 10, n)]


def _expect_full(c, g, deg):
    assert g.n == g.parent_nid.numel() == c["node_cap"], "the capacity case has spare rows: it lost its point"


def _expect_hub(c, g, deg):
    assert int(deg.max()) > c["max_degree"], "no row above max_degree: the clamp is not exercised"
    assert int(deg.max()) >= 64 + 16, "the hub row does not span every lane group of the gather"


def _expect_table_limit(c, g, deg):
    assert (c["max_degree"] + 1) * c["emb"] == EMB_LDS_FLOATS


def _expect_kdim(k):
    def f(c, g, deg):
        assert c["pos"] + c["emb"] + 1 == k and (c["max_degree"] + 1) * c["emb"] <= EMB_LDS_FLOATS
    return f


def _expect_stripped(c, g, deg):
    assert g.n == 198 and all(int(deg[r]) == 0 for r in c["strip"]) and int((deg == 0).sum()) == len(c["strip"])


def _expect_seed_last(c, g, deg):
    sizes = torch.tensor(c["sizes"])
    sl = torch.tensor(c["seed_local"])
    assert bool((sl < sizes).all()) and int((sl == sizes - 1).sum()) >= 1 and bool((sl != 0).all())


_EMPTIES = [0, 5, 0, 0, 30, 1, 0, 63, 2, 0, 9, 9, 9, 0, 1, 1, 7, 0]
_STAR = [90, 40]

CASES = {
    # ---- the 64-row tile, one graph: BatchNorm and pooling see a single segment
    "one_graph_20": case([20], 1),
    "one_graph_64": case([64], 202),
    "one_graph_65": case([65], 3),
    # ---- node_cap == N: the speculative first-tile requests clamp (cap_row)
    "cap_equals_n_128": case([60, 68], 404, node_cap=128, expect=_expect_full),
    "cap_equals_n_73": case([20, 50, 3], 105, node_cap=73, expect=_expect_full),
    "rows_hint_1": case([20, 50, 3], 206, rows_hint=1),
    # ---- the readout's groups of 16 graphs: nread = ((B + 15) / 16 * (L + 1) + 3) / 4
    "readout_b15": case(_small(15, 15), 107),
    "readout_b16": case(_small(16, 16), 8),
    "readout_b17": case(_small(17, 17), 9),
    "readout_b33": case(_small(33, 33), 510),
    # ---- empty and one-node graphs, also first and last
    "empty_and_single_graphs": case(_EMPTIES, 711),
    # ---- rows without edges on both sides of every tile border
    "stripped_rows_at_tile_borders": case([4] * 32 + [70], 4212, strip=(0, 63, 64, 127, 128, 197), expect=_expect_stripped),
    # ---- a hub row that crosses every lane group of the gather, forward and backward; the max_degree clamp
    "hub_max_degree_4": case(_STAR, 813, star=True, max_degree=4, expect=_expect_hub),
    "hub_max_degree_2": case(_STAR, 414, star=True, max_degree=2, expect=_expect_hub),
    "hub_table_10240_floats": case(_STAR, 515, star=True, max_degree=639, expect=_expect_table_limit),
    # ---- depth: 1, 2 and GCC_GIN_MAX_LAYERS GIN layers
    "layers_2": case([20, 50, 3], 116, layers=2),
    "layers_3": case([20, 50, 3], 117, layers=3),
    "layers_9": case([20, 50, 3], 818, layers=9),
    # ---- the input column layout: both branches of gin_bwd_emb_kernel at widths that are no multiple of 4
    "cols_32_31": case([20, 50, 3], 119, pos=32, emb=31, max_degree=329, expect=_expect_kdim(64)),
    "cols_30_17": case([20, 50, 3], 20, pos=30, emb=17, max_degree=64, expect=_expect_kdim(48)),
    "cols_32_5": case([20, 50, 3], 221, pos=32, emb=5, max_degree=64, expect=_expect_kdim(38)),
    "cols_6_16": case([20, 50, 3], 22, pos=6, emb=16, max_degree=64, expect=_expect_kdim(23)),
    "cols_2_1": case([20, 50, 3], 23, pos=2, emb=1, max_degree=64, expect=_expect_kdim(4)),
    # ---- the fine-tuning path on whole graphs: the seed is not local node 0 (once it is a graph's last node)
    "seed_local": case([20, 50, 3], 24, seed_local=[19, 7, 2], expect=_expect_seed_last),
    # ---- a second backward of the same pass with accumulate=True leaves twice the gradient
    "accumulate": case([20, 50, 3], 725, accumulate=True),
}


def build_graphs(c):
    """-> (node_off, row_ptr, col_idx, degrees) as int64 arrays: symmetric, free of self loops, no graph complete (the pair of a
    graph's first and last node is never an edge; a two-node graph has none).  A graph of three or more nodes is a path plus about
    half as many random chords; ``star``: the first graph is a star around its node 0 with a path through the leaves.  The rows
    in ``strip`` lose every edge."""
    rng = np.random.default_rng(1000 + c["seed"])
    sizes = c["sizes"]
    node_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(node_off[-1])
    adj = [set() for _ in range(n)]

    def link(u, v):
        adj[u].add(v)
        adj[v].add(u)

    for b, s in enumerate(sizes):
        o = int(node_off[b])
        if c["star"] and b == 0:
            for v in range(1, s):
                link(o, o + v)
            for v in range(1, s - 1):
                link(o + v, o + v + 1)
            continue
        if s < 3:
            continue
        for v in range(s - 1):
            link(o + v, o + v + 1)
        for _ in range(s // 2):
            u, v = (int(x) for x in rng.integers(0, s, 2))
            if u != v and {u, v} != {0, s - 1}:
                link(o + u, o + v)
    for r in c["strip"]:
        for v in adj[r]:
            adj[v].discard(r)
        adj[r] = set()
    for b, s in enumerate(sizes):                    # the input condition: symmetric, no self loop, never complete
        o = int(node_off[b])
        edges = sum(len(adj[o + v]) for v in range(s))
        assert all(o <= u < o + s and u != o + v and (o + v) in adj[u] for v in range(s) for u in adj[o + v])
        assert s < 2 or edges < s * (s - 1), f"graph {b} is complete"
    deg = np.array([len(a) for a in adj], dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col_idx = np.concatenate([np.array(sorted(a), dtype=np.int64) for a in adj])
    return node_off, row_ptr, col_idx, deg


def build_batch(tier, c):
    """-> (the tier's batch, the oracle's arguments, degrees)"""
    node_off, row_ptr, col_idx, deg = build_graphs(c)
    n = int(node_off[-1])
    pos = torch.nn.functional.normalize(torch.randn(n, c["pos"], generator=torch.Generator().manual_seed(c["seed"])), dim=1)
    view = dict(node_off=torch.from_numpy(node_off), row_ptr=torch.from_numpy(row_ptr), col_idx=torch.from_numpy(col_idx),
                pos_undirected=pos)
    g = CpuBatch(view, node_cap=c["node_cap"])
    c["expect"](c, g, deg)
    dev = tier.batch(g)
    if c["seed_local"] is not None:
        dev.seed_local = tier.to(torch.tensor(c["seed_local"], dtype=torch.int32))
    return dev, (view["node_off"], view["row_ptr"], view["col_idx"], pos), deg


def build_models(tier, c):
    """-> (GraphEncoder on the tier in train mode, the oracle in fp32, the oracle in float64), one state"""
    torch.manual_seed(c["seed"])
    oracle = E.OracleGraphEncoder(positional_embedding_size=c["pos"], max_degree=c["max_degree"], degree_embedding_size=c["emb"],
                                  output_dim=H, node_hidden_dim=H, num_layers=c["layers"], norm=True)
    for mod in oracle.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.3)
    oracle.degree_embedding.weight.data.normal_(0, 1)
    model = GraphEncoder(positional_embedding_size=c["pos"], max_node_freq=16, max_edge_freq=16, max_degree=c["max_degree"],
                         freq_embedding_size=16, degree_embedding_size=c["emb"], output_dim=H, node_hidden_dim=H,
                         edge_hidden_dim=H, num_layers=c["layers"], num_step_set2set=6, num_layer_set2set=3, norm=True,
                         gnn_model="gin", degree_input=True)
    assert not model.wide and not model.is_padded()
    model.load_state_dict(oracle.state_dict())
    model = tier.to(model)
    model.train()
    o32, o64 = copy.deepcopy(oracle), copy.deepcopy(oracle).double()
    o32.train()
    o64.train()
    return model, o32, o64


def _run_oracle(o, args, keep, dfeat, seed_local, dt):
    """-> (feat, {name: gradient}, the smallest |output| of any BatchNorm: each of them feeds a ReLU)"""
    o.zero_grad()
    near = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: near.append(float(out.detach().abs().min())))
             for m in o.gnn.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    feat = o(args[0], args[1], args[2], args[3].to(dt), dropout_masks=keep.to(dt), seed_local=seed_local)
    for h in hooks:
        h.remove()
    feat.backward(dfeat.to(dt))
    return feat.detach(), {n: p.grad for n, p in o.named_parameters()}, min(near)


def reference(c, args, o32, o64):
    """the oracle's side of a case: the dropout masks and d feat of its seed, the fp32 and the float64 run.  Asserts the input
    conditions that only the reference can show: no float64 pre-activation lies within the forward bar's absolute tolerance
    (2e-5, on BatchNorm outputs of order one) of a ReLU kink -- a kernel that meets the forward bar may put such an element on
    either side, and its whole upstream gradient follows (seen on the emulator build: one element at 7.3e-6 in float64, every
    gradient of the kernels 2e-2 of its scale from float64 and 3e-5 from float64 with that one mask flipped, while torch's fp32
    run stayed at 9e-5) -- and torch's fp32 gradients are inside the bar against float64."""
    B, L = len(c["sizes"]), c["layers"]
    gen = torch.Generator().manual_seed(100 + c["seed"])
    keep = (torch.rand(L, B, H, generator=gen) >= 0.5).float().contiguous()
    dfeat = torch.randn(B, H, generator=gen)
    f32, g32, _ = _run_oracle(o32, args, keep, dfeat, c["seed_local"], torch.float32)
    f64, g64, near = _run_oracle(o64, args, keep, dfeat, c["seed_local"], torch.float64)
    assert near >= TOL["atol"], f"BAD INPUT: a float64 pre-activation is {near:.1e} from a ReLU kink (closer than {TOL['atol']:.0e})"
    bad32 = []
    for pname, ref in g64.items():
        if ref is not None:
            e32 = float((g32[pname].double() - ref).abs().max())
            if not e32 <= grad_bar(pname, ref)[1]:
                bad32.append(f"d {pname}: {e32:.3e} (bar {grad_bar(pname, ref)[1]:.3e})")
    assert not bad32, "BAD INPUT, not a kernel error -- torch's fp32 run of the oracle is outside the bar against float64: " \
                      + "; ".join(bad32)
    return keep, dfeat, f32, g32, f64, g64


def check_case(tier, name):
    """-> dict(feat=(kernel, fp32 reference) worst absolute error, grad=(kernel, fp32 reference) worst share of the largest entry)"""
    c = CASES[name]
    L = c["layers"]
    g, args, deg = build_batch(tier, c)
    model, o32, o64 = build_models(tier, c)
    keep, dfeat, f32, g32, f64, g64 = reference(c, args, o32, o64)

    eng = tier.gin_engine()
    eng.rows_hint = c["rows_hint"]
    keep_dev, dfeat_dev = tier.to(keep), tier.to(dfeat)
    p, buf = eng.make_pass(model, g, training=True, keep=keep_dev)
    assert p.node_cap == (c["node_cap"] or int(args[0][-1]) + 37) and p.w.num_gin_layers == L - 1
    eng.forward([p])
    eng.backward(model, p, buf, dfeat_dev)
    if c["accumulate"]:
        eng.backward(model, p, buf, dfeat_dev, accumulate=True)
    tier.sync()
    times = 2.0 if c["accumulate"] else 1.0

    # ---- forward: the embeddings, and every BatchNorm's running statistics after the pass
    feat = buf["feat"].detach().cpu().double()
    feat_err, feat_err32 = float((feat - f64).abs().max()), float((f32.double() - f64).abs().max())
    torch.testing.assert_close(feat, f64, msg=lambda m: f"{name}: feat: {m}", **TOL)
    s64 = o64.state_dict()
    stats = 0
    for k, v in model.state_dict().items():
        if "running_" in k:
            torch.testing.assert_close(v.cpu().double(), s64[k], msg=lambda m, k=k: f"{name}: {k}: {m}", **STAT_TOL)
            stats += 1
        elif "num_batches" in k:
            assert torch.equal(v.cpu(), s64[k]), f"{name}: {k}"
    assert stats == 2 * 3 * (L - 1)

    # ---- gradients against float64, the reference condition on torch's fp32 run at the same bar
    worst, worst32, who, who32 = 0.0, 0.0, None, None
    bad = []
    for pname, prm in model.named_parameters():
        ref = g64[pname]
        if ref is None:
            assert prm.grad is None or float(prm.grad.abs().sum()) == 0.0, f"{name}: {pname} has a gradient the oracle does not give"
            continue
        assert prm.grad is not None and prm.grad.shape == prm.shape, f"{name}: {pname}"
        scale, atol = grad_bar(pname, ref)
        err = float((prm.grad.cpu().double() / times - ref).abs().max())
        e32 = float((g32[pname].double() - ref).abs().max())
        assert err == err, f"{name}: d {pname} holds a NaN"
        if err / scale > worst:
            worst, who = err / scale, pname
        if e32 / scale > worst32:
            worst32, who32 = e32 / scale, pname
        if err > atol:
            bad.append(f"d {pname}: {err:.3e} (bar {atol:.3e})")
    print(f"gin edge {name}: feat {feat_err:.2e} (torch fp32 {feat_err32:.2e}) absolute; worst gradient entry vs float64 "
          f"{worst:.2e} ({who}) | torch fp32 {worst32:.2e} ({who32}) of the tensor's largest entry")
    assert not bad, f"{name}: gradients from the float64 oracle: " + "; ".join(bad)
    return dict(feat=(feat_err, feat_err32), grad=(worst, worst32))
