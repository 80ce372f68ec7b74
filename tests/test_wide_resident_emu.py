"""GraphEncoder.resident_eval / gcc_ginw_embed on the lock-step emulator: the eval-mode embedding of a wide GIN encoder in
one call (feature rows in bf16 -> LDS-resident bf16 layers, block by block over 128 nodes -> f32 readout, normalisation
and the mean of the views) against tests/wide_resident_reference.py, through the product's own host code
(gcc_amd.gin_wide.WideResidentEngine with the emulator library injected).  The device tier is
tests/test_wide_resident_gpu.py."""
import argparse
import copy
import os

import numpy as np
import pytest
import torch

from gcc_amd.encoder import GraphEncoder
from gcc_amd.gin_wide import WideResidentEngine
from tests import wide_resident_reference as R
from tests.hipemu.emu_driver import emu_ginw_forward, emu_lib
from tests.hipemu.emu_encoder import CpuBatch

# view q: an isolated node without edges, a partial 16-row fragment, the exact 128 boundary, one row into the block path
SIZES_Q = [1, 2, 37, 128, 129, 61]
SIZES_K = [3, 128, 1, 130, 16, 64]


def cpu_ptr(t):
    return 0 if t is None else t.data_ptr()


def emu_resident_engine():
    return WideResidentEngine(lib=emu_lib(), ptr=cpu_ptr)


def wide_model(hidden, out, num_layers, norm, seed=0, **kw):
    torch.manual_seed(seed)
    args = dict(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=512, freq_embedding_size=16,
                degree_embedding_size=16, output_dim=out, node_hidden_dim=hidden, edge_hidden_dim=hidden, num_layers=num_layers,
                num_step_set2set=6, num_layer_set2set=3, norm=norm, gnn_model="gin", degree_input=True)
    args.update(kw)
    enc = GraphEncoder(**args)
    if enc.gnn_model == "gin":
        R.randomize_running_stats(enc, seed + 1)
    enc.eval()
    enc.resident_eval = True
    enc._resident_engine = emu_resident_engine()
    return enc


def make_views(seed, mult, seeded, sizes=(SIZES_Q, SIZES_K)):
    rng = np.random.default_rng(seed)
    views = []
    for s in sizes:
        g = CpuBatch(R.ego_views(rng, s))                   # node capacity N + 37
        g.edge_multiplicity = mult
        if seeded:
            g.seed_local = torch.from_numpy(rng.integers(0, np.asarray(s)).astype(np.int32))
        views.append(g)
    return views


def embed(enc, views):
    out = enc.embed_views(views[0], views[-1])
    assert enc.resident_engine().check_status() == 0
    return out


# every value of every parameter, and both row-block paths, in four calls (an emulated call takes seconds)
@pytest.mark.parametrize("hidden,out,num_layers,mult,seeded,norm,two_views", [
    (256, 256, 3, 2, True, True, True),
    (96, 72, 3, 1, False, False, True),
    (128, 128, 5, 2, False, True, False),
    (96, 72, 3, 2, True, False, False),
])
def test_resident_embedding_meets_both_bars(hidden, out, num_layers, mult, seeded, norm, two_views):
    enc = wide_model(hidden, out, num_layers, norm, seed=hidden + mult)
    views = make_views(7 + hidden, mult, seeded)
    if not two_views:
        views = views[:1]
    got = embed(enc, views)
    assert tuple(got.shape) == (len(SIZES_Q), out) and got.dtype == torch.float32
    R.check_bars(got.numpy(), enc, views, mult, label=f"hidden {hidden} mult {mult}")
    # padding: channels the model does not have are exactly zero in the pooled sums the readout read
    pooled = enc.resident_engine().pooled
    d_in = 32 + 16 + 1
    assert tuple(pooled.shape) == (len(views), len(SIZES_Q), num_layers, 256)
    assert not pooled[:, :, 0, d_in:].any() and not pooled[:, :, 1:, hidden:].any()
    assert pooled[:, :, 1:, :hidden].abs().sum() > 0


def test_multiplicity_equals_physically_duplicated_entries():
    """edge multiplicity 2 is, bit for bit, the CSR with every entry twice and multiplicity 1 (the counters are integers;
    the degree feature is row length x multiplicity either way)"""
    enc = wide_model(96, 72, 3, True, seed=5)
    views = make_views(11, 2, True, sizes=([2, 37, 129], [130, 1, 16]))
    got = embed(enc, views)
    pooled = enc.resident_engine().pooled.clone()
    dup = []
    for g in views:
        d = copy.copy(g)
        d.row_ptr = g.row_ptr * 2
        d.col_idx = torch.repeat_interleave(g.col_idx, 2)
        d.edge_multiplicity = 1
        dup.append(d)
    got_dup = embed(enc, dup)
    assert torch.equal(enc.resident_engine().pooled, pooled) and torch.equal(got, got_dup)


def test_ginw_forward_is_bit_identical_to_the_recorded_outputs():
    """count_neighbours took an increment argument; gcc_ginw_forward passes 1: rows and pooled sums of one batch of
    tests/test_gin_wide_emu.py's generator (a subgraph over 128 nodes in it) equal the outputs recorded before the change
    (tests/golden/make_ginw_forward_golden.py)"""
    from tests.golden.make_ginw_forward_golden import OUT, golden_inputs

    node_off, row_ptr, col_idx, x, layers, digest = golden_inputs()
    want = np.load(OUT)
    assert str(want["inputs_sha256"]) == digest, "the generator no longer draws the recorded inputs"
    rows, pooled, status = emu_ginw_forward(node_off, row_ptr, col_idx, x, layers, scratch=True)
    assert status == 0
    assert np.array_equal(rows, want["rows"]) and np.array_equal(pooled.view(np.uint32), want["pooled"].view(np.uint32))


def test_fold_cache_follows_in_place_updates_and_load_state_dict():
    enc = wide_model(96, 72, 3, True, seed=9)
    views = make_views(13, 1, False, sizes=([5, 20], [9, 3]))
    first = embed(enc, views)
    fold = enc.resident_engine()._fold[1]
    assert enc.resident_engine().folded(enc) is fold                       # nothing changed: the fold is reused
    with torch.no_grad():                                                   # what an optimizer step does
        enc.gnn.ginlayers[1].apply_func.mlp.linears[0].weight.mul_(-1.5)
        enc.gnn.batch_norms[0].running_mean.add_(0.25)                      # a buffer
    second = embed(enc, views)
    assert enc.resident_engine()._fold[1] is not fold
    assert not torch.allclose(first, second, rtol=1e-2, atol=1e-3)
    R.check_bars(second.numpy(), enc, views, 1, label="after the in-place update")
    other = wide_model(96, 72, 3, True, seed=10)
    enc.load_state_dict(other.state_dict())
    third = embed(enc, views)
    R.check_bars(third.numpy(), enc, views, 1, label="after load_state_dict")
    torch.testing.assert_close(third, embed(other, views), rtol=0, atol=0)


def test_refusals_by_name():
    views = make_views(3, 1, False, sizes=([4, 6], [5, 2]))

    def refused(enc, pattern):
        enc.resident_eval = True
        with pytest.raises(NotImplementedError, match=pattern):
            enc.embed_views(views[0], views[1])

    refused(wide_model(300, 256, 3, True), "widths up to 256")                          # hidden
    refused(wide_model(128, 320, 3, True), "widths up to 256")                          # output
    refused(wide_model(128, 128, 3, True, positional_embedding_size=250), "widths up to 256")     # input: 250 + 16 + 1
    deep = wide_model(128, 128, 9, True)
    deep.gnn.ginlayers.append(copy.deepcopy(deep.gnn.ginlayers[-1]))                    # (the constructor stops at 8)
    refused(deep, "at most 8 GIN layers")
    refused(wide_model(32, 32, 3, True, gnn_model="gat"), "GAT")
    refused(wide_model(64, 64, 3, True), "not a wide GIN encoder")
    training = wide_model(128, 128, 3, True)
    training.train()
    refused(training, "training-mode BatchNorm")
    ema_style = wide_model(128, 128, 3, True)                                           # train.py:357-365: eval() with BatchNorm in train()
    for m in ema_style.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.train()
    refused(ema_style, "training-mode BatchNorm")
    # default: the attribute is off and embed_views is what it was
    plain = GraphEncoder(positional_embedding_size=32, degree_embedding_size=16, output_dim=128, node_hidden_dim=128, num_layers=3,
                         gnn_model="gin", degree_input=True)
    assert plain.resident_eval is False and plain._resident_engine is None


def one_graph_batch(copies, mult):
    """3 nodes; row 0 lists node 1 ``copies`` times"""
    view = dict(node_off=torch.tensor([0, 3]), row_ptr=torch.tensor([0, copies, copies + 1, copies + 1]),
                col_idx=torch.tensor([1] * copies + [0]), pos_undirected=torch.randn(3, 32, generator=torch.Generator().manual_seed(0)))
    g = CpuBatch(view)
    g.edge_multiplicity = mult
    return g


def test_a_count_above_256_is_reported_by_name():
    enc = wide_model(96, 72, 3, True, seed=2)
    g = one_graph_batch(300, 1)
    enc.embed_views(g, g)
    with pytest.raises(RuntimeError, match="more than 256 times"):
        enc.resident_engine().check_status()
    assert enc.resident_engine().check_status() == 0                        # (the word was cleared)
    g = one_graph_batch(128, 2)                                             # exactly 256: exact in bf16, served
    got = embed(enc, [g])
    R.check_bars(got.numpy(), enc, [g], 2, label="count 256")
    g = one_graph_batch(129, 2)                                             # 258
    enc.embed_views(g, g)
    with pytest.raises(RuntimeError, match="more than 256 times"):
        enc.resident_engine().check_status()


def test_c_abi_refuses_bad_arguments():
    from gcc_amd import _cabi

    lib = emu_lib()
    assert lib.gcc_ginw_embed_workspace_bytes(0, 4) < 0 and lib.gcc_ginw_embed_workspace_bytes(100, 0) < 0
    assert lib.gcc_ginw_embed_workspace_bytes(1000, 4) >= 1000 * 256 * 2 * 3
    a = _cabi.GccGinwEmbedArgs(num_views=3, batch_size=1, num_layers=1)
    status = np.zeros(1, dtype=np.int32)
    assert lib.gcc_ginw_embed(a, status.ctypes.data, None) != 0
    assert b"gcc_ginw_embed" in lib.gcc_last_error()


class EmuPipeline:
    """generate.py's pipeline seam on the emulator: sampler, positional embedding and engines built on the emulator library"""

    device = torch.device("cpu")

    def __init__(self):
        self.batches = []

    def node_dataset(self, **kw):
        from gcc_amd.datasets import NodeClassificationDataset
        from gcc_amd.graph import max_nodes_out_degree_table
        from tests.hipemu.emu_driver import EmuGraph, emu_sample_batch

        (rp, ci), mult, rw_hops, restart_prob, B = kw["graph"], kw["edge_multiplicity"], kw["rw_hops"], kw["restart_prob"], kw["batch_size"]
        ltab = max_nodes_out_degree_table(int(np.diff(rp).max()), rw_hops, restart_prob, mult)
        g = EmuGraph(rp, ci, rw_hops=rw_hops, restart_prob=restart_prob, ltab=ltab)
        self.node_cap = B * (g.lmax + 1)

        def sample_fn(first_id, seeds):
            res, status, used = emu_sample_batch(g, B, 3, first_id, seeds=seeds)
            assert status == 0 and (used == seeds).all()
            out = []
            for r in res:
                n = len(r["parent_nid"])
                b = CpuBatch(dict(node_off=torch.from_numpy(r["node_off"].astype(np.int64)),
                                  row_ptr=torch.from_numpy(r["row_ptr"].astype(np.int64)),
                                  col_idx=torch.from_numpy(r["col_idx"].astype(np.int64)),
                                  pos_undirected=torch.zeros(n, 32)), node_cap=self.node_cap)
                b.parent_nid[:n] = torch.from_numpy(r["parent_nid"])
                out.append(b)
            self.batches.append(tuple(out))
            return tuple(out)

        return NodeClassificationDataset(sample_fn=sample_fn, **kw), self.node_cap, lambda: None

    def posemb(self, batch_size, node_cap, size, seed):
        from gcc_amd.posemb import DevicePosEmb

        return DevicePosEmb(batch_size, node_cap, size, device="cpu", lib=emu_lib(), ptr=cpu_ptr, max_views=2, num_buffers=4)

    def place(self, model):
        from gcc_amd.encoder_wide import WideGinEngine

        model._wide_engine = WideGinEngine(lib=emu_lib(), ptr=cpu_ptr)
        model._resident_engine = emu_resident_engine()
        self.model = model
        return model


def write_checkpoint(tmp_path, hidden, model="gin"):
    opt = argparse.Namespace(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=512, freq_embedding_size=16,
                             degree_embedding_size=16, hidden_size=hidden, num_layer=3, set2set_iter=6, set2set_lstm_layer=3, norm=True,
                             model=model, rw_hops=24, subgraph_size=64, restart_prob=0.8, seed=0, model_folder=str(tmp_path / "out"))
    from gcc_amd.encoder import encoder_from_opt

    torch.manual_seed(hidden)
    enc = encoder_from_opt(opt)
    if model == "gin":
        R.randomize_running_stats(enc, 4)
    path = tmp_path / "ckpt.pth"
    torch.save(dict(opt=opt, model=enc.state_dict(), epoch=1), path)
    return str(path), opt


def generate_args(tmp_path, load_path, **kw):
    from tests.test_generate_emu import _write_edgelist

    _write_edgelist(tmp_path, n=20, extra=24, seed=2)
    a = argparse.Namespace(load_path=load_path, dataset="toy", gpu=None, edgelist=str(tmp_path / "toy.edgelist"), nodelabel=None,
                           graph_npz=None, graphs_npz=None, tudataset=None, edge_multiplicity=0, batch_size=16, wide_eval="resident")
    a.__dict__.update(kw)
    return a


def test_generate_py_wide_eval_resident_end_to_end(tmp_path):
    """generate.py --wide-eval resident on an edge list (multiplicity 2) with a hidden-96 checkpoint: the saved array
    against the reference on the batches the run sampled, at both bars"""
    import generate

    load_path, opt = write_checkpoint(tmp_path, 96)
    pipe = EmuPipeline()
    generate.main(generate_args(tmp_path, load_path), pipeline=pipe)
    emb = np.load(os.path.join(opt.model_folder, "toy.npy"))
    assert emb.shape == (20, 96) and pipe.model.resident_eval and len(pipe.batches) == 2
    assert pipe.batches[0][0].edge_multiplicity == 2
    e_rule, e_truth = [], []
    for q, k in pipe.batches:
        lo = len(e_rule) and sum(len(e) for e in e_rule)
        got = emb[lo: lo + q.valid]
        ref = R.reference_embedding(pipe.model, [q, k], 2, bf16=True)[: q.valid]
        truth = R.reference_embedding(pipe.model, [q, k], 2, bf16=False)[: q.valid]
        e_rule.append(R.graph_errors(got, ref))
        e_truth.append(R.graph_errors(got, truth))
    e_rule, e_truth = np.concatenate(e_rule), np.concatenate(e_truth)
    print("generate.py rows: worst error vs the bf16 rule %.2e, vs the truth %.2e" % (e_rule.max(), e_truth.max()))
    assert len(e_rule) == 20 and (e_rule < R.BAR_RULE).all() and (e_truth < R.BAR_TRUTH).all()


def test_generate_py_refuses_the_flag_for_other_checkpoints(tmp_path):
    import generate

    load_path, _ = write_checkpoint(tmp_path, 64)
    with pytest.raises(SystemExit, match="wide GIN checkpoints"):
        generate.main(generate_args(tmp_path, load_path), pipeline=EmuPipeline())
    load_path, _ = write_checkpoint(tmp_path, 32, model="gat")
    with pytest.raises(SystemExit, match="wide GIN checkpoints"):
        generate.main(generate_args(tmp_path, load_path), pipeline=EmuPipeline())
