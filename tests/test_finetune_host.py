"""Host side of --finetune (CPU): the fold split, the device-style F1, the labelled datasets' batches, the resume override
and the checkpoint keys, each against the reference's own definition."""
import argparse
import types

import numpy as np
import pytest
import torch


def test_fold_split_is_sklearns_stratified_kfold():
    from sklearn.model_selection import StratifiedKFold

    from gcc_amd.finetune_main import fold_split

    rng = np.random.default_rng(0)
    labels = rng.integers(0, 4, 137).tolist()
    for seed in (0, 7):
        ref = list(StratifiedKFold(n_splits=10, shuffle=True, random_state=seed).split(np.zeros(len(labels)), labels))
        for fold in range(10):
            tr, te = fold_split(labels, fold, seed)
            assert np.array_equal(tr, ref[fold][0]) and np.array_equal(te, ref[fold][1])
    with pytest.raises(AssertionError):
        fold_split(labels, 10, 0)


def test_device_style_f1_equals_sklearn_micro_f1():
    from sklearn.metrics import f1_score

    rng = np.random.default_rng(1)
    for C in (2, 3, 5):
        y, pred = rng.integers(0, C, 200), rng.integers(0, C, 200)
        correct, valid = int((y == pred).sum()), len(y)
        assert abs(correct / valid - f1_score(y, pred, average="micro")) < 1e-12


def test_graph_dataset_labels_padding_and_posemb_reuse():
    from gcc_amd.datasets import GraphClassificationDatasetLabeled
    from gcc_amd.graphgen import powerlaw_graph

    graphs = [powerlaw_graph(10 + i, 30 + 2 * i, i) for i in range(7)]
    ds = GraphClassificationDatasetLabeled(graphs=graphs, labels=[i % 2 for i in range(7)], batch_size=4, device="cpu")
    calls = []
    # the positional embedding of every graph is computed once (the reference's self.dict): a counting stand-in
    ds._embed_all = lambda: (calls.append(1), setattr(ds, "_pos", torch.arange(int(ds.first[-1]), dtype=torch.float32)
                                                      .unsqueeze(1).repeat(1, 32)))[-1]
    got = list(ds.batches([6, 2, 5, 0, 1]))
    assert len(got) == 2 and len(calls) == 1
    g, y = got[1]
    assert got[0][1].tolist() == [0, 0, 1, 0] and y.tolist() == [1, -1, -1, -1]    # graphs 6 2 5 0 | 1, then padding
    no = g.node_off.tolist()
    assert no[1] == no[2] == no[3] == no[4] == graphs[1][0].shape[0] - 1   # empty padding subgraphs
    assert g.pos_undirected[0, 0] == ds.first[1]                           # graph 1's cached embedding rows
    assert got[0][0].pos_undirected[0, 0] == ds.first[6]
    list(ds.batches([3]))
    assert len(calls) == 1


def test_node_dataset_uses_constant_max_nodes_and_argmax_labels(monkeypatch):
    import gcc_amd.datasets as D

    made = {}

    class FakeGraph:
        def __init__(self, rp, ci, rw_hops, restart_prob, device, ltab):
            made["ltab"] = ltab

    class FakeSampler:
        node_cap = 100

        def __init__(self, graph, B, run_seed, num_buffers):
            pass

        def sample(self, first, seeds):
            made.setdefault("seeds", []).append(seeds.tolist())
            B = len(seeds)
            g = types.SimpleNamespace(batch_size=B, node_off=torch.arange(B + 1, dtype=torch.int32) * 3,
                                      edge_off=torch.arange(B + 1, dtype=torch.int32) * 5,
                                      row_ptr=torch.arange(3 * B + 1, dtype=torch.int32), col_idx=torch.arange(5 * B, dtype=torch.int32))
            return g, None

    class FakePosEmb:
        def __init__(self, *a, **k):
            pass

        def __call__(self, g):
            made["embedded"] = made.get("embedded", 0) + 1

    import gcc_amd.graph
    import gcc_amd.posemb
    import gcc_amd.sampler
    monkeypatch.setattr(gcc_amd.graph, "DeviceGraph", FakeGraph)
    monkeypatch.setattr(gcc_amd.sampler, "DeviceRWRSampler", FakeSampler)
    monkeypatch.setattr(gcc_amd.posemb, "DevicePosEmb", FakePosEmb)
    from gcc_amd.graphgen import powerlaw_graph

    rp, ci = powerlaw_graph(50, 200, 0)
    n = len(rp) - 1
    y = np.zeros((n, 3), dtype=np.float32)
    y[np.arange(n), np.arange(n) % 3] = 1
    ds = D.NodeClassificationDatasetLabeled(graph=(rp, ci), labels=y, rw_hops=17, batch_size=4, device="cpu")
    assert np.all(made["ltab"] == 17) and len(made["ltab"]) == int(np.diff(rp).max()) + 1
    (g0, y0), (g1, y1) = list(ds.batches([7, 8, 9, 10, 11]))
    assert made["seeds"] == [[7, 8, 9, 10], [11, 0, 0, 0]]
    assert y0.tolist() == [7 % 3, 8 % 3, 9 % 3, 10 % 3] and y1.tolist() == [11 % 3, -1, -1, -1]
    assert g1.node_off.tolist() == [0, 3, 3, 3, 3] and g1.valid == 1       # padding rows are empty subgraphs
    assert made["embedded"] == 2                                           # one view per batch
    # the default multiplicity 2 (an edge list's DGL graph): every CSR entry twice, the batch then counts as simple
    assert g0.edge_multiplicity == 1 and g0.col_idx[:4].tolist() == [0, 0, 1, 1] and g0.row_ptr[:3].tolist() == [0, 2, 4]


def test_resume_override_semantics():
    import train
    from gcc_amd.finetune_main import apply_resume

    pre = train.parse_option(["--moco", "--nce-k", "128", "--rw-hops", "64", "--learning_rate", "0.01", "--epochs", "100"])
    cli = train.parse_option(["--finetune", "--dataset", "imdb-binary", "--epochs", "3", "--batch-size", "8", "--fold-idx", "4",
                              "--cv", "--resume", "x.pth", "--num-workers", "3"])
    cli.gpu = 0
    a = apply_resume(cli, pre)
    # train.py:490-503: these come from the command line, everything else from the checkpoint
    assert (a.fold_idx, a.gpu, a.finetune, a.resume, a.cv, a.dataset, a.epochs, a.batch_size) == (4, 0, True, "x.pth", True,
                                                                                                 "imdb-binary", 3, 8)
    assert a.num_workers == 0                                              # graph classification: :500-502
    assert (a.moco, a.nce_k, a.rw_hops, a.learning_rate) == (True, 128, 64, 0.01)


def test_checkpoint_keys_are_the_references():
    import inspect

    from gcc_amd import finetune_main

    src = inspect.getsource(finetune_main.main_finetune)
    assert '{"opt": args, "model": model.state_dict(), "contrast": contrast.state_dict(),' in src
    assert '"optimizer": optimizer.state_dict(), "epoch": epoch}' in src
    assert "output_layer" not in src.split("state = {")[1].split("}")[0]   # the head is not saved (train.py:747-786)
