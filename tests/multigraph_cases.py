"""Multigraph test cases shared by tests/test_multigraph_emu.py and tests/test_multigraph_gpu.py: parallel edges are
repeated, adjacent entries of sorted CSR rows (gcc_amd.ingest.multigraph_csr).  Every builder is deterministic."""
import numpy as np
import torch

from gcc_amd.ingest import multigraph_csr
from oracle import posemb as P

HID = 32
WEIGHTS = (1, 1, 2, 3, 7)


def expand(a, rng, weights=WEIGHTS):
    """scipy CSR of a simple symmetric graph -> (row_ptr, col_idx) int32 with every undirected edge ``rng.choice(weights)``
    times."""
    up = __import__("scipy.sparse").sparse.triu(a, 1).tocoo()
    pairs = np.stack([up.row, up.col], axis=1).astype(np.int64)
    w = np.asarray(weights, dtype=np.int64)[rng.randint(0, len(weights), len(pairs))]
    return multigraph_csr(pairs, w, a.shape[0])


def view_of(rp, ci, node_off=None):
    n = len(rp) - 1
    return dict(node_off=torch.tensor([0, n] if node_off is None else list(node_off)),
                row_ptr=torch.from_numpy(np.asarray(rp, dtype=np.int64)), col_idx=torch.from_numpy(np.asarray(ci, dtype=np.int64)))


def sparse_power_graph(n, rng):
    """The sparse recipe of test_sparse_graph_beyond_the_dense_classes_is_solved_by_the_block_class (power 0.6, ~6 entries
    per node, connected) at ``n`` nodes -> scipy CSR"""
    import scipy.sparse as sp

    w = 1.0 / np.arange(1, n + 1) ** 0.6
    pr = np.minimum(1.0, 3.0 * np.outer(w, w) / (w.mean() ** 2 * n))
    up = np.triu(rng.rand(n, n) < pr, 1)
    up[np.arange(n - 1), np.arange(1, n)] = True
    a = sp.csr_matrix((up | up.T).astype(np.float64))
    a.sort_indices()
    return a


# size -> (graph seed, deflated-size class).  Seeds chosen so that the float64 gap below the wanted subspace is > 1e-3
# (asserted by every test that uses them) and the deflated size falls into the class under test.
EIG_CASES = {40: (3, (1, 48)), 56: (3, (49, 64)), 100: (3, (65, 128)), 200: (3, (129, 384)), 420: (3, (385, 704))}


def eig_view(n):
    """One weighted view for the dense class of size ``n``: the graph first, then the weights, from one RandomState."""
    from tests.test_posemb_emu import skewed_dense_graph

    seed = EIG_CASES[n][0]
    rng = np.random.RandomState(seed)
    if n <= 128:
        a = skewed_dense_graph(n, seed=seed)
    else:
        a = sparse_power_graph(n, rng)
    rp, ci = expand(a, rng)
    assert (np.diff(ci)[np.diff(np.repeat(np.arange(n), np.diff(rp))) == 0] == 0).any()      # there ARE repeated entries
    return view_of(rp, ci)


def float64_gap(view, b=0):
    """s[-k] - s[-k-1] of the float64 multigraph matrix of subgraph ``b``: the Gram check of _check runs only above 1e-3"""
    no = view["node_off"].numpy()
    rp, ci = view["row_ptr"].numpy(), view["col_idx"].numpy()
    lo, hi = no[b], no[b + 1]
    n = hi - lo
    k = min(n - 2, HID)
    M = P.normalized_adjacency(rp[lo:hi + 1] - rp[lo], ci[rp[lo]:rp[hi]] - lo).toarray()
    s = np.linalg.eigvalsh(M)
    return float(s[-k] - s[-k - 1]) if n - k - 1 >= 0 else np.inf


def deflation_view():
    """One batch for the deflation rules under multiplicity: (pairs, weights) per block.
    0: twin leaves on a hub that also has tripled edges;  1: three stalks with single hub edges, a look-alike stalk whose
    hub edge is doubled and a node tied to its only neighbour by two edges, all on one hub;  2: a spider (k = n - 2);
    3: a spider whose first leg's hub edge is doubled (two stalks + the look-alike, k = n - 2);  4: blocks 0 and 1 on a
    core large enough for the 65..128 class."""
    def core(n0, n, p, rng, wts=(1, 1, 2, 3)):
        e = [(n0 + i, n0 + i + 1) for i in range(n - 1)]
        e += [(n0 + i, n0 + j) for i in range(n) for j in range(i + 2, n) if rng.rand() < p]
        return e, [int(wts[rng.randint(len(wts))]) for _ in e]

    rng = np.random.RandomState(5)
    blocks = []
    # 0: hub 0, core 1..6 (hub - 1 tripled, hub - 2 tripled, hub - 3 single), twin leaves 7..10
    e, w = core(1, 6, 0.4, rng)
    e += [(0, 1), (0, 2), (0, 3)] + [(0, 7 + i) for i in range(4)]
    w += [3, 3, 1] + [1] * 4
    blocks.append((11, e, w))
    # 1: hub 0, core 1..5; stalks (6,7) (8,9) (10,11) single; look-alike (12,13) with 0 - 12 doubled; node 14 tied to 0 twice;
    #    node 15 tied to core node 2 twice
    e, w = core(1, 5, 0.5, rng)
    e += [(0, 1), (0, 3)]
    w += [2, 1]
    for a in (6, 8, 10):
        e += [(0, a), (a, a + 1)]
        w += [1, 1]
    e += [(0, 12), (12, 13), (0, 14), (2, 15)]
    w += [2, 1, 2, 2]
    blocks.append((16, e, w))
    # 2: the spider of stalky_view, simple
    blocks.append((7, [(0, 1), (1, 2), (0, 3), (3, 4), (0, 5), (5, 6)], [1] * 6))
    # 3: a spider of four legs, the first hub edge doubled
    blocks.append((9, [(0, 1), (1, 2), (0, 3), (3, 4), (0, 5), (5, 6), (0, 7), (7, 8)], [2, 1, 1, 1, 1, 1, 1, 1]))
    # 4: a 90-node core; hub 0 with 5 twin leaves, tripled core edges, 4 stalks, a look-alike and a doubled pendant
    e, w = core(0, 90, 0.06, rng, wts=(1, 1, 2, 3, 5))
    nxt = 90
    e += [(0, nxt + i) for i in range(5)]
    w += [1] * 5
    nxt += 5
    for _ in range(4):
        e += [(0, nxt), (nxt, nxt + 1)]
        w += [1, 1]
        nxt += 2
    e += [(0, nxt), (nxt, nxt + 1), (0, nxt + 2)]
    w += [2, 1, 2]
    nxt += 3
    blocks.append((nxt, e, w))
    node_off, pairs, weights = [0], [], []
    for n, e, w in blocks:
        o = node_off[-1]
        pairs += [(o + i, o + j) for i, j in e]
        weights += w
        node_off.append(o + n)
    rp, ci = multigraph_csr(np.array(pairs), np.array(weights), node_off[-1])
    return view_of(rp, ci, node_off)


def weighted_parent(rp, ci, rng, weights=(1, 1, 1, 2, 3, 5)):
    """A simple symmetric parent CSR -> the multigraph with every undirected edge weighted from ``weights``"""
    import scipy.sparse as sp

    n = len(rp) - 1
    a = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    return expand(a, rng, weights)


# ---- eval encoders on repeated entries (two subgraphs, 90 and 40 nodes, copies 1..5)
def encoder_view(seed=0, sizes=(90, 40), pos_dim=32):
    """-> the dict CpuBatch takes: sparse connected subgraphs, every undirected edge 1..5 times, unit-norm random rows in
    ``pos_undirected`` (the encoders are checked on their own here, not behind the eigensolver)"""
    rng = np.random.RandomState(seed)
    pairs, weights, node_off = [], [], [0]
    for n in sizes:
        o = node_off[-1]
        e = {(i, i + 1) for i in range(n - 1)} | {(0, j) for j in range(2, n, 3)}        # a hub row: the long runs are there
        while len(e) < 3 * n:
            a, b = sorted(rng.randint(0, n, 2))
            if a != b:
                e.add((a, b))
        e = sorted(e)
        pairs += [(o + a, o + b) for a, b in e]
        weights += list(rng.randint(1, 6, len(e)))
        node_off.append(o + n)
    rp, ci = multigraph_csr(np.array(pairs), np.array(weights), node_off[-1])
    pos = torch.nn.functional.normalize(torch.randn(node_off[-1], pos_dim, generator=torch.Generator().manual_seed(seed)), dim=1)
    view = view_of(rp, ci, node_off)
    view["pos_undirected"] = pos
    return view


def _oracle_args(view):
    return view["node_off"].long(), view["row_ptr"].long(), view["col_idx"].long(), view["pos_undirected"]


def check_fused_eval_and_chain(tier, rtol, atol):
    """gcc_gin_eval_fused and the 15-launch eval chain of the hidden-64 encoder against oracle/encoder.py on the same CSR"""
    from oracle import encoder as E
    from tests.hipemu.emu_encoder import CpuBatch, emu_engine, reference_encoder
    from tests.wide_resident_reference import randomize_running_stats

    torch.manual_seed(3)
    oracle = E.OracleGraphEncoder()
    randomize_running_stats(oracle, 4)
    model = reference_encoder()
    model.load_state_dict(oracle.state_dict())
    model = tier.to(model)
    if tier.name == "emu":
        model._engine = emu_engine()
    model.eval()
    oracle.eval()
    view = encoder_view()
    q = tier.batch(CpuBatch(view))
    with torch.no_grad():
        ref = oracle(*_oracle_args(view))
        for fused in (True, False):
            model.fused_eval = fused
            got = model(q)
            tier.sync()
            print("fused" if fused else "chain", "max abs error vs the oracle %.2e" % float((got.cpu() - ref).abs().max()))
            torch.testing.assert_close(got.cpu(), ref, rtol=rtol, atol=atol)
        model.fused_eval = True
        torch.testing.assert_close(model.embed_views(q, q).cpu(), ref, rtol=rtol, atol=atol)


def check_any_width_chain(tier, rtol, atol):
    """the any-width eval chain (hidden 96 -> 80, three layers) against oracle/encoder.py on the same CSR"""
    from oracle import encoder as E
    from tests.hipemu.emu_encoder import CpuBatch
    from tests.wide_edges_check import encoder
    from tests.wide_resident_reference import randomize_running_stats

    torch.manual_seed(5)
    model = encoder(96, 80, 3)
    randomize_running_stats(model, 6)
    oracle = E.OracleGraphEncoder(node_hidden_dim=96, output_dim=80, num_layers=3)
    oracle.load_state_dict(model.state_dict())
    model = tier.to(model)
    model._wide_engine = tier.wide_engine()
    model.eval()
    oracle.eval()
    view = encoder_view(seed=1)
    q = tier.batch(CpuBatch(view))
    with torch.no_grad():
        got, ref = model(q), oracle(*_oracle_args(view))
    tier.sync()
    print("any-width chain max abs error vs the oracle %.2e" % float((got.cpu() - ref).abs().max()))
    torch.testing.assert_close(got.cpu(), ref, rtol=rtol, atol=atol)


def check_resident_embed(tier):
    """gcc_ginw_embed (bf16 layers resident in LDS) on repeated entries: copies x edge_multiplicity <= 256 is served inside the
    project's two bars for this path (tests/wide_resident_reference.py: 1e-3 against the bf16 rule, 2e-2 against float64
    -- bf16 layers cannot meet an f32 tolerance); more sets its status bit."""
    import pytest

    from tests import wide_resident_reference as R
    from tests.hipemu.emu_encoder import CpuBatch
    from tests.wide_edges_check import encoder

    torch.manual_seed(7)
    enc = encoder(96, 72, 3)
    R.randomize_running_stats(enc, 8)
    enc = tier.to(enc).eval()
    enc.resident_eval = True
    if tier.name == "emu":
        from tests.test_wide_resident_emu import emu_resident_engine

        enc._resident_engine = emu_resident_engine()
    view = encoder_view(seed=2)
    for mult in (1, 2):
        g = CpuBatch(view)
        g.edge_multiplicity = mult
        q = tier.batch(g)
        q.edge_multiplicity = mult
        got = enc.embed_views(q, q)
        tier.sync()
        assert enc.resident_engine().check_status() == 0
        R.check_bars(got.cpu().numpy(), enc, [q], mult, label=f"multigraph rows x {mult}")
    # 60 copies of one edge x multiplicity 5 = 300 > 256: refused by name, not rounded
    rp, ci = multigraph_csr(np.array([[0, 1], [1, 2]]), np.array([60, 1]), 3)
    small = view_of(rp, ci)
    small["pos_undirected"] = torch.nn.functional.normalize(torch.randn(3, 32, generator=torch.Generator().manual_seed(0)), dim=1)
    g = CpuBatch(small)
    q = tier.batch(g)
    q.edge_multiplicity = 5
    enc.embed_views(q, q)
    tier.sync()
    with pytest.raises(RuntimeError, match="more than 256 times"):
        enc.resident_engine().check_status()


def check_gat_forward(tier, rtol, atol):
    """GAT forward: every parallel edge is its own softmax term (DGL's edge softmax on the multigraph), against the float64
    restatement on the same CSR"""
    from gcc_amd.encoder import GatEngine
    from tests.gat_check import gat_encoder
    from tests.gat_reference import forward_of, params_of
    from tests.hipemu.emu_encoder import CpuBatch

    enc = gat_encoder(hidden=32, heads=4, layers=2, T=2, Lr=2, pos=8, deg_emb=8, max_degree=64)
    view = encoder_view(seed=3, pos_dim=8)
    with torch.no_grad():
        ref = forward_of(enc, params_of(enc), view, mult=1)
    enc = tier.to(enc)
    q = tier.batch(CpuBatch(view))
    eng = GatEngine(**tier._kw())
    out = eng.forward(enc, q)[0]
    tier.sync()
    print("GAT forward max abs error vs float64 %.2e" % float((out.double().cpu() - ref).abs().max()))
    torch.testing.assert_close(out.double().cpu(), ref, rtol=rtol, atol=atol)


# ---- the whole path on a weighted co-author network: reader -> sampler -> positional embedding -> encoder
def ss_graph_files(folder):
    """the toy ``.graph`` / ``.dict`` pair the reference was executed on (tests/golden/ssgraph_reference.json) -> paths"""
    import json
    import os

    ref = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ssgraph_reference.json")))
    paths = os.path.join(str(folder), "toy.graph"), os.path.join(str(folder), "toy.dict")
    open(paths[0], "w").write(ref["graph"])
    open(paths[1], "w").write(ref["dict"])
    return paths


def check_whole_path(tier, folder, rtol, atol, B=16, rw_hops=24, run_seed=3):
    """generate.py's loop (test_moco) over the toy network as the multigraph the reference builds: node sets, rows and
    columns of every batch against the C oracle on the expanded CSR, embeddings against oracle/encoder.py on the batches
    with the double insertion expanded too."""
    from gcc_amd import ingest
    from gcc_amd.datasets import NodeClassificationDataset
    from gcc_amd.generate import test_moco
    from gcc_amd.posemb import DevicePosEmb
    from oracle import encoder as E
    from oracle import sampler as O
    from tests.hipemu.emu_encoder import CpuBatch, emu_engine, reference_encoder
    from tests.wide_resident_reference import randomize_running_stats

    d = ingest.read_ss_graph(*ss_graph_files(folder), csr=True)
    rp, ci, mult = d["row_ptr"], d["col_idx"], d["edge_multiplicity"]
    kw = dict(rw_hops=rw_hops, restart_prob=0.8, positional_embedding_size=HID, graph=(rp, ci), edge_multiplicity=mult,
              batch_size=B, multigraph=True)
    if tier.name == "emu":
        from gcc_amd.graph import max_nodes_out_degree_table
        from tests.hipemu.emu_driver import EmuGraph, emu_lib, emu_sample_batch

        g = EmuGraph(rp, ci, rw_hops=rw_hops, restart_prob=0.8, contract_checked=False,
                     ltab=max_nodes_out_degree_table(int(np.diff(rp).max()), rw_hops, 0.8, mult))
        node_cap = B * (g.lmax + 1)

        def sample_fn(first_id, seeds):
            res, status, used = emu_sample_batch(g, B, run_seed, first_id, seeds=seeds, edge_cap=8 * B * (g.lmax + 1) ** 2)
            assert status == 0 and (used == seeds).all()
            out = []
            for r in res:
                n = len(r["parent_nid"])
                b = CpuBatch(dict(node_off=torch.from_numpy(r["node_off"].astype(np.int64)),
                                  row_ptr=torch.from_numpy(r["row_ptr"].astype(np.int64)),
                                  col_idx=torch.from_numpy(r["col_idx"].astype(np.int64)),
                                  pos_undirected=torch.zeros(n, HID)), node_cap=node_cap)
                b.parent_nid[:n] = torch.from_numpy(r["parent_nid"])
                out.append(b)
            return tuple(out)

        ds = NodeClassificationDataset("toy", sample_fn=sample_fn, **kw)
        pe = DevicePosEmb(B, node_cap, HID, device="cpu", lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr(),
                          max_views=2, num_buffers=4)
    else:
        ds = NodeClassificationDataset("toy", run_seed=run_seed, device="cuda", **kw)
        assert ds.graph.multigraph and not ds.graph.contract_checked and ds.graph.hub_index is None
        pe = DevicePosEmb(B, ds.sampler.node_cap, HID, device="cuda", seed=run_seed, max_views=2, num_buffers=2)
    torch.manual_seed(1)
    oracle = E.OracleGraphEncoder()
    randomize_running_stats(oracle, 2)
    model = reference_encoder()
    model.load_state_dict(oracle.state_dict())
    model = tier.to(model)
    if tier.name == "emu":
        model._engine = emu_engine()
    model.fused_eval = True
    kept = []

    def host(b):
        n = int(b.node_off[b.batch_size])
        e = int(b.row_ptr[n])
        return dict(node_off=b.node_off[: b.batch_size + 1].cpu().long(), row_ptr=b.row_ptr[: n + 1].cpu().long(),
                    col_idx=b.col_idx[:e].cpu().long(), parent_nid=b.parent_nid[:n].cpu().numpy(),
                    pos=b.pos_undirected[:n].cpu().clone(), valid=b.valid)

    class Spy:                                               # copies every batch once the loop is done with it
        def __iter__(self):
            for q, k in ds:
                yield q, k
                tier.sync()
                kept.append((host(q), host(k)))

    emb = test_moco(Spy(), model, pe)
    if tier.name == "gpu":
        ds.sampler.check_status()
    pe.check_status()
    assert emb.shape == (len(rp) - 1, 64) and len(kept) == 3
    c = O.COracle()
    deg = np.diff(rp)
    oracle.eval()
    ref = []
    for i, views in enumerate(kept):
        seeds = np.zeros(B, dtype=np.int32)
        seeds[: views[0]["valid"]] = np.arange(i * B, i * B + views[0]["valid"])
        L = ds.ltab[deg[seeds]].astype(np.int32)
        fs = []
        for view, b in enumerate(views):
            r = c.sample_batch(rp, ci, seeds, L, view, run_seed, i * B, O.restart_threshold(0.8))
            assert np.array_equal(b["parent_nid"], r["parent_nid"]) and np.array_equal(b["node_off"].numpy(), r["node_off"])
            assert np.array_equal(b["row_ptr"].numpy(), r["row_ptr"]) and np.array_equal(b["col_idx"].numpy(), r["col_idx"])
            with torch.no_grad():
                fs.append(oracle(b["node_off"], mult * b["row_ptr"], torch.repeat_interleave(b["col_idx"], mult), b["pos"]))
        ref.append(((fs[0] + fs[1]) / 2)[: views[0]["valid"]])
    ref = torch.cat(ref)
    print("whole path max abs error vs the oracle %.2e" % float((emb - ref).abs().max()))
    torch.testing.assert_close(emb, ref, rtol=rtol, atol=atol)
