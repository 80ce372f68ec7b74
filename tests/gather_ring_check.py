"""The neighbour gather's ring of row requests (gather_tile, gcc_amd/csrc/encoder_common.h) at the sizes where it can go wrong,
through the C ABI, for both tiers (tests/test_gather_ring_emu.py: the wave64 emulator; tests/test_gather_ring_gpu.py: the device).

The ring changed WHEN a feature row is requested, not one addition: every case must give the bits that the commit before it
wrote on the same tier (tests/golden/gather_ring_bits_<tier>.npz, tests/golden/make_gather_ring_golden.py), and -- so that a
wrong recording cannot hide a wrong kernel -- the neighbour sums must agree with float64 sums to 1e-5 of the largest entry.

A tile is 64 rows, its E edges are split over 16 lane groups in chunks of ceil(E / 16), a group sums its chunk in halves of 4
rows (two halves in flight), and the targets arrive in rounds of 16 edges.  The tiles here put the chunk at 0, 1, 3, 4, 5, 7, 8,
9, 15, 16, 17, 32 and 33: the half, the pair of halves, the 16-edge round, and one to each side of them.

Recorded per case: agg of layers 0 and 1 (gin_in_kernel without and with its BatchNorm transform), z1 and the statistics of
layer 0, agg of layer 0 at edge multiplicity 2, U of layer 0 (gin_bwd_c_kernel's last launch) and the degree-embedding gradient
(all that leaves gin_bwd_emb_kernel's gather of the input-feature gradient); for the one graph of more than 320 nodes the
embedding of gcc_gin_eval_fused at multiplicity 1 and 2 (the general kernel of encoder_eval.hip).  Float64 restatements: agg of
layers 0 and 1, z1, the degree-embedding gradient, the eval embedding (the oracle); U rests on the recording alone.  Of the per-node arrays one
column per lane of a lane group is kept (column 4 t + (t & 3) of lane t: a lane's four columns are one load and one add4), which
keeps the two recordings at a few hundred KB."""
import os

import numpy as np
import torch

TILE = 64
H = 64
CHUNKS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 32, 33)
COLS = np.array([4 * t + (t & 3) for t in range(16)])
WALK_TILES = 33                    # against the smallest grid (32 workgroups): one workgroup walks on to a second tile
REL = 1e-5                         # (set by the issue) the longest row here has 77 edges: f32 additions stay below 77 * 2^-24 = 4.6e-6 of the largest entry


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _degrees(rng, rows, edges):
    """``edges`` edges over ``rows`` rows, some rows empty"""
    d = np.zeros(rows, dtype=np.int64)
    live = rng.permutation(rows)[: max(1, (3 * rows) // 4)]
    for _ in range(edges):
        d[live[rng.integers(len(live))]] += 1
    return d


def tile_of_chunk(rng, chunk, rows=TILE):
    """a tile whose 16 lane groups get ``chunk`` edges each, the last ones fewer (E = 16 chunk - 5 is no multiple of 16)"""
    return _degrees(rng, rows, max(16 * chunk - 5, 0))


def hub_tile():
    """one row holds every edge: its sum crosses all 16 groups, every group's first and last slot is that row"""
    d = np.zeros(TILE, dtype=np.int64)
    d[20] = 16 * 5 - 3
    return d


def spans_tile():
    """chunk 4 (E = 64).  Row 1: edges 2-5 = groups 0 and 1; row 2: edges 6-13 = groups 1, 2 and 3; rows 4, 5: empty where
    group 4's chunk starts (edge 16); row 7: empty in the middle of it; row 9: empty where it ends (edge 20)"""
    d = [2, 4, 8, 2, 0, 0, 3, 0, 1, 0] + [1] * 44 + [0] * 10
    assert len(d) == TILE and sum(d) == 64
    return np.array(d, dtype=np.int64)


def groups_of_row(deg, r):
    """the lane groups that hold edges of row ``r`` of the tile with degrees ``deg``"""
    rp = np.r_[0, np.cumsum(deg)]
    chunk = (rp[-1] + 15) // 16
    return sorted(set(int(e // chunk) for e in range(rp[r], rp[r + 1])))


def view_of(tiles, seed, graphs=2):
    """tiles (degree arrays; all but the last 64 rows long) -> one batch; targets anywhere in the batch"""
    rng = np.random.default_rng(seed)
    assert all(len(t) == TILE for t in tiles[:-1]) and 1 <= len(tiles[-1]) <= TILE
    deg = np.concatenate(tiles)
    n = len(deg)
    rp = np.r_[0, np.cumsum(deg)].astype(np.int64)
    ci = rng.integers(0, n, int(rp[-1])).astype(np.int64)
    cut = sorted(set([0, n] + [int(x) for x in np.linspace(0, n, graphs + 1)[1:-1]])) if n > 1 else [0, n]
    pos = torch.randn(n, 32, generator=torch.Generator().manual_seed(seed)) * 0.3
    return dict(node_off=torch.tensor(cut), row_ptr=torch.from_numpy(rp), col_idx=torch.from_numpy(ci), pos_undirected=pos)


def cases():
    """name -> (view, rows_hint, kind); kind "train" or "eval\""""
    rng = np.random.default_rng(11)
    out = {}
    for i in range(0, 12, 3):
        cs = CHUNKS[i:i + 3]
        out["chunks_%d_%d_%d" % cs] = (view_of([tile_of_chunk(rng, c) for c in cs], 20 + i), None, "train")
    out["chunk_33_last_row_alone"] = (view_of([tile_of_chunk(rng, 33), np.array([3])], 40), None, "train")
    out["chunk_9_last_63_rows"] = (view_of([tile_of_chunk(rng, 9), tile_of_chunk(rng, 5, 63)], 41), None, "train")
    out["hub_spans_no_edges"] = (view_of([hub_tile(), spans_tile(), np.zeros(TILE, dtype=np.int64)], 42), None, "train")
    out["one_row"] = (view_of([np.array([0])], 43, graphs=1), None, "train")
    walk = [_degrees(rng, TILE, int(rng.integers(100, 330))) for _ in range(WALK_TILES - 1)] + [_degrees(rng, 5, 9)]
    out["walk_on"] = (view_of(walk, 44, graphs=7), 1, "train")
    out["wide_embedding"] = (view_of([hub_tile(), tile_of_chunk(rng, 3), tile_of_chunk(rng, 33, 40)], 46), None, "train")
    out["eval_large_graph"] = (symmetric_graph(330, 45), None, "eval")
    return out


def symmetric_graph(n, seed):
    """one graph of ``n`` nodes: a cycle, 2 n random pairs and a hub with 100 neighbours, symmetric (the oracle takes a node's
    degree from the entries that point at it, the kernels from its row: only a symmetric graph lets the two be compared)"""
    rng = np.random.default_rng(seed)
    a = np.r_[np.arange(n), rng.integers(0, n, 2 * n), np.zeros(100, dtype=np.int64)]
    b = np.r_[(np.arange(n) + 1) % n, rng.integers(0, n, 2 * n), rng.choice(np.arange(1, n), 100, replace=False)]
    k = a != b
    e = np.unique(np.r_[a[k] * n + b[k], b[k] * n + a[k]])
    rows, cols = e // n, e % n
    rp = np.r_[0, np.cumsum(np.bincount(rows, minlength=n))].astype(np.int64)
    pos = torch.randn(n, 32, generator=torch.Generator().manual_seed(seed)) * 0.3
    return dict(node_off=torch.tensor([0, n]), row_ptr=torch.from_numpy(rp), col_idx=torch.from_numpy(cols.astype(np.int64)),
                pos_undirected=pos)


def recorded_rows(name, n):
    """the rows of a per-node array that are recorded (walk_on: the last tiles, those a workgroup walks on to among them)"""
    return slice(max(0, n - 3 * TILE - 5), n) if name == "walk_on" else slice(0, n)


class Tier:
    """``batch(view) -> batch``, ``engine() -> GinEngine``, ``dev``: where tensors live"""

    def __init__(self, tier, lib=None):
        from gcc_amd.encoder import GinEngine
        from tests.hipemu.emu_encoder import CpuBatch

        self.tier = tier
        if tier == "emu":
            from tests.hipemu.emu_driver import emu_lib

            self.dev = "cpu"
            lib = lib if lib is not None else emu_lib()
            self.engine = lambda: GinEngine(lib=lib, ptr=lambda t: 0 if t is None else t.data_ptr())
            self.batch = lambda view: CpuBatch(view)
        else:
            from tests.test_encoder_gpu import gpu_batch

            self.dev = "cuda"
            self.engine = lambda: GinEngine(lib=lib)
            self.batch = gpu_batch


WIDE_EMB = {"wide_embedding": 24}      # degree-embedding columns of a case (default 16); above 16 gin_bwd_emb_kernel gathers 16 bytes a lane


def _model(dev, emb=16):
    """the encoder of train.py's default flags (tests/hipemu/emu_encoder.py: reference_encoder), ``emb`` degree-embedding columns"""
    from gcc_amd.encoder import GraphEncoder

    torch.manual_seed(1)
    return GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16,
                        max_degree=512 if emb <= 16 else 300,      # (the kernel's table holds 10,240 floats)
                        freq_embedding_size=16, degree_embedding_size=emb, output_dim=64, node_hidden_dim=64,
                        edge_hidden_dim=64, num_layers=5, num_step_set2set=6, num_layer_set2set=3,
                        norm=True, gnn_model="gin", degree_input=True).to(dev)


def oracle_eval(model, view, mult):
    """the eval-mode embedding by the float64 oracle on the CSR with every entry ``mult`` times (tests/test_encoder_emu.py)"""
    from oracle import encoder as E

    oracle = E.OracleGraphEncoder()
    oracle.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    oracle = oracle.double().eval()
    rp, ci = view["row_ptr"].numpy(), view["col_idx"].numpy()
    with torch.no_grad():
        ref = oracle(view["node_off"], torch.from_numpy(mult * rp), torch.from_numpy(np.repeat(ci, mult)),
                     view["pos_undirected"].double())
    return ref.numpy()


def run_case(T, name, view, hint, kind):
    """-> dict of numpy arrays (full width; :func:`record` cuts them down)"""
    n, B = int(view["node_off"][-1]), len(view["node_off"]) - 1
    out = {}
    if kind == "eval":
        for mult in (1, 2):
            model = _model(T.dev)
            model.eval()
            eng = T.engine()
            b = T.batch(view)
            b.edge_multiplicity = mult
            p, buf = eng.make_pass(model, b, training=False)
            eng.eval_fused([p])
            out["feat_m%d" % mult] = buf["feat"].cpu().numpy().copy()
            out["ref_m%d" % mult] = oracle_eval(model, view, mult)
        return out
    keep = (torch.rand(5, B, H, generator=torch.Generator().manual_seed(3)) > 0.5).float().to(T.dev)
    d = torch.randn(B, H, generator=torch.Generator().manual_seed(4)).to(T.dev)
    model = _model(T.dev, WIDE_EMB.get(name, 16))
    model.train()
    eng = T.engine()
    eng.rows_hint = hint
    b = T.batch(view)
    p, buf = eng.make_pass(model, b, training=True, keep=keep)
    eng.forward([p])
    out["x0"] = buf["x0"][:n].cpu().numpy().copy()
    out["agg0"], out["agg1"] = (buf["agg"][i][:n].cpu().numpy().copy() for i in (0, 1))
    out["z1"] = buf["z1"][0][:n].cpu().numpy().copy()
    out["z2"] = buf["z2"][0][:n].cpu().numpy().copy()
    lay = model.gnn.ginlayers[0].apply_func
    f64 = lambda t: t.detach().double().cpu().numpy()
    out["w0"], out["b0"] = f64(lay.mlp.linears[0].weight), f64(lay.mlp.linears[0].bias)
    out["bn"] = [(f64(m.weight), f64(m.bias), m.eps) for m in (lay.bn, model.gnn.batch_norms[0])]
    out["stats0"] = buf["stats"][0, 0].cpu().numpy().copy()                 # [replicas][2][64] fp64: layer 0, linears.0's output
    eng.backward(model, p, buf, d)
    cap = p.node_cap
    ws = next(v for k, v in eng._bufs.items() if k[0] == "bwd")
    act = cap * H                                                           # floats per activation block (encoder_bwd.hip: bwd_layout)
    wsf = ws.view(torch.float32)
    out["U"] = wsf[:act].view(cap, H)[:n].cpu().numpy().copy()
    out["D"] = wsf[3 * act:4 * act].view(cap, H)[:n].cpu().numpy().copy()   # dagg of layer 0: what gin_bwd_emb_kernel gathers
    L = len(model.gnn.ginlayers)
    g_at = (4 + 2 * L) * act
    blk = ((L + 1) * B * H * 4 + 255) // 256 * 64                           # floats of G, 256-byte aligned
    out["dpooled0"] = wsf[g_at + blk:g_at + blk + B * H].view(B, H).cpu().numpy().copy()
    out["demb"] = model.degree_embedding.weight.grad.detach().cpu().numpy().copy()
    # the multigraph path of gin_in_kernel (forward only: the backward pass refuses a multiplicity)
    model2 = _model(T.dev, WIDE_EMB.get(name, 16))
    model2.train()
    eng2 = T.engine()
    eng2.rows_hint = hint
    b2 = T.batch(view)
    b2.edge_multiplicity = 2
    p2, buf2 = eng2.make_pass(model2, b2, training=True, keep=keep)
    eng2.forward([p2])
    out["agg0_m2"] = buf2["agg"][0][:n].cpu().numpy().copy()
    out["x0_m2"] = buf2["x0"][:n].cpu().numpy().copy()                      # (degrees double with the multiplicity: other features)
    return out


PER_NODE = ("agg0", "agg1", "z1", "U", "agg0_m2")


def record(name, res):
    """what the golden files hold of a case's results"""
    rec = {}
    for k, v in res.items():
        if k in PER_NODE:
            rec[k] = bits(v[recorded_rows(name, len(v))][:, COLS])
        elif k in ("feat_m1", "feat_m2", "demb"):
            rec[k] = bits(v)
        elif k == "stats0":
            rec[k] = np.ascontiguousarray(v).view(np.uint64)
    return rec


def golden_path(tier):
    return os.path.join(os.path.dirname(__file__), "golden", "gather_ring_bits_%s.npz" % tier)


def float64_checks(name, view, res):
    """the gathers against float64 sums, REL of the largest entry"""
    rp, ci = view["row_ptr"].numpy(), view["col_idx"].numpy()
    n = len(rp) - 1
    row = np.repeat(np.arange(n), np.diff(rp))

    def nbr_sum(x):
        s = np.zeros((n, x.shape[1]))
        np.add.at(s, row, x[ci].astype(np.float64))
        return s

    def close(got, want, what, floor=0.0):
        err, scale = np.abs(got - want).max(initial=0.0), max(np.abs(want).max(initial=0.0), floor)
        print(name, what, "max error %.3g, largest entry %.3g" % (err, scale))
        assert err <= REL * max(scale, 1e-30), (name, what, err, scale)

    x0 = res["x0"].astype(np.float64)
    close(res["agg0"], x0 + nbr_sum(res["x0"]), "agg of layer 0")
    # linears.0 on the exact-f32 matrix cores: z1 = agg W0^T + b0 (49 products a column)
    w0 = res["w0"]
    close(res["z1"][:, :w0.shape[0]], res["agg0"].astype(np.float64)[:, :w0.shape[1]] @ w0.T + res["b0"], "z1 of layer 0")
    # gin_in_kernel of layer 1: h = relu(bn_c(relu(bn_b(z2)))) on the batch statistics (biased variance), then h_v + sum h_u
    # (the kernel's affine is x s + (b - m s) in f32, s = g / sqrt(var + eps): it rounds at the size of the terms that cancel,
    #  |m s|, not of the result -- with one row in the batch the result is 0 and |m s| is not -- so that size counts as an entry)
    h, cancel = res["z2"].astype(np.float64), 0.0
    for g, b, eps in res["bn"]:
        sc = g[:h.shape[1]] / np.sqrt(h.var(0) + eps)
        cancel = max(cancel, float(np.abs(h.mean(0) * sc).max()))
        h = np.maximum((h - h.mean(0)) * sc + b[:h.shape[1]], 0.0)
    close(res["agg1"], h + nbr_sum(h), "agg of layer 1", floor=cancel)
    close(res["agg0_m2"], res["x0_m2"].astype(np.float64) + 2.0 * nbr_sum(res["x0_m2"]), "agg of layer 0, multiplicity 2")
    # gin_bwd_emb_kernel: dx0 = (I + A) dagg_0 + dpooled_0[graph]; d emb[min(deg, max)] += dx0[:, 32:48]
    no = view["node_off"].numpy()
    gid = np.repeat(np.arange(len(no) - 1), np.diff(no))
    dx0 = res["D"].astype(np.float64) + nbr_sum(res["D"]) + res["dpooled0"].astype(np.float64)[gid]
    want = np.zeros(res["demb"].shape)
    np.add.at(want, np.minimum(np.diff(rp), want.shape[0] - 1), dx0[:, 32:32 + want.shape[1]])
    close(res["demb"], want, "degree-embedding gradient")


def check_case(T, name):
    view, hint, kind = cases()[name]
    res = run_case(T, name, view, hint, kind)
    if kind == "train":
        float64_checks(name, view, res)
    else:                                            # the float64 oracle, at the bound of the other encoder tests (rtol 1e-4, atol 2e-5)
        for m in (1, 2):
            got, want = res["feat_m%d" % m].astype(np.float64), res["ref_m%d" % m]
            print(name, "multiplicity", m, "max error %.3g" % np.abs(got - want).max())
            assert np.all(np.abs(got - want) <= 2e-5 + 1e-4 * np.abs(want)), (name, m)
        assert np.abs(res["feat_m1"] - res["feat_m2"]).max() > 1e-4      # the multiplicity matters
    z = np.load(golden_path(T.tier))
    rec = record(name, res)
    assert rec, name
    for k, v in rec.items():
        want = z["%s__%s" % (name, k)]
        assert v.shape == want.shape and np.array_equal(v, want), (name, k, int((v != want).sum()), "entries differ")


def check_cases_cross_their_boundaries():
    """the tiles have the chunks, spans and empty rows the cases are named for (both tiers run the same cases)"""
    cs = cases()
    seen = set()
    for name, (view, hint, kind) in cs.items():
        rp = view["row_ptr"].numpy()
        n = len(rp) - 1
        for t0 in range(0, n, TILE):
            e = int(rp[min(t0 + TILE, n)] - rp[t0])
            seen.add((e + 15) // 16)
    assert set(CHUNKS) <= seen, sorted(seen)
    hub = hub_tile()
    assert groups_of_row(hub, 20) == list(range(16)) and hub.sum() == hub[20]
    sp = spans_tile()
    assert groups_of_row(sp, 1) == [0, 1] and groups_of_row(sp, 2) == [1, 2, 3]
    rp = np.r_[0, np.cumsum(sp)]
    assert rp[4] == rp[5] == rp[6] == 16 and rp[7] == rp[8] == 19 and rp[9] == rp[10] == 20     # empty rows: start, middle, end of group 4's chunk
    v = cs["hub_spans_no_edges"][0]["row_ptr"].numpy()
    assert v[3 * TILE] == v[2 * TILE]                                                            # a tile with no edges at all
    assert len(cs["chunk_33_last_row_alone"][0]["row_ptr"]) - 1 == TILE + 1
    assert len(cs["chunk_9_last_63_rows"][0]["row_ptr"]) - 1 == TILE + 63
    assert len(cs["walk_on"][0]["row_ptr"]) - 1 > 32 * TILE and cs["walk_on"][1] == 1            # more tiles than the 32 workgroups of the smallest grid
    assert len(cs["eval_large_graph"][0]["row_ptr"]) - 1 > 320 and len(cs["eval_large_graph"][0]["node_off"]) == 2
