"""``--tu-parse`` of train.py, generate.py and ``python -m gcc_amd.tasks.graph_classification`` (CPU tier): the default is the
host reader everywhere, the flag is refused by name where it cannot be served, ``--resume`` keeps it, and the whole-graph datasets
take ``corpus=`` in place of ``graphs=``."""
import argparse

import numpy as np
import pytest
import torch


def test_defaults_are_the_host_reader(monkeypatch, tmp_path):
    import train
    from gcc_amd import ingest
    from gcc_amd.tasks import _common, graph_classification
    from tests import tu_ingest_check as C

    assert train.parse_option([]).tu_parse == "host" and train.parse_option(["--tudataset", "d"]).tu_parse == "host"
    assert train.parse_option(["--tudataset", "d", "--tu-parse", "device"]).tu_parse == "device"
    assert _common.generate_namespace("c.pth", "imdb-binary", "cpu", 8, tudataset="d").tu_parse == "host"
    assert _common.generate_namespace("c.pth", "imdb-binary", "cpu", 8, tu_parse="device", tudataset="d").tu_parse == "device"
    assert "--tu-parse" in open(train.__file__.replace("train.py", "generate.py")).read()
    # the task reads its labels with the host reader unless told otherwise
    pairs, indicator, labels = C.dataset([C.TRIANGLE, C.path(3)], [4, 9])
    folder = C.write_files(tmp_path / "d", pairs, indicator, labels)
    seen = []
    real = ingest.read_tudataset
    monkeypatch.setattr(ingest, "read_tudataset", lambda folder, name: seen.append(name) or real(folder, name))
    a = argparse.Namespace(tudataset=folder, graphs_npz=None, dataset=C.NAME, device="cpu", tu_parse="host")
    assert graph_classification.load_labels(a).tolist() == [0, 1] and seen == [C.NAME]
    del a.tu_parse                                                  # (a namespace from before the flag)
    assert graph_classification.load_labels(a).tolist() == [0, 1]


def test_train_refuses_tu_parse_without_tudataset_and_with_the_host_batcher(capsys):
    import train

    with pytest.raises(SystemExit):
        train.parse_option(["--tu-parse", "device"])
    assert "--tu-parse device says where the files of --tudataset are parsed" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_option(["--tu-parse", "device", "--tudataset", "d", "--graph-batcher", "host"])
    assert "--tu-parse device builds the resident corpus of the device batcher: not with --graph-batcher host" in capsys.readouterr().err


def test_task_refuses_tu_parse_without_tudataset_and_on_the_cpu(capsys, tmp_path):
    from gcc_amd.tasks import graph_classification

    np.save(tmp_path / "e.npy", np.zeros((2, 4), dtype=np.float32))
    common = ["--dataset", "imdb-binary", "--emb-path", str(tmp_path / "e.npy"), "--tu-parse", "device"]
    with pytest.raises(SystemExit):
        graph_classification.main(common + ["--graphs-npz", "g.npz"])
    assert "--tu-parse device says where the files of --tudataset are parsed" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        graph_classification.main(common + ["--tudataset", str(tmp_path), "--device", "cpu"])
    assert "--tu-parse device needs a GPU --device" in capsys.readouterr().err


def test_load_labelled_and_generate_refuse_by_name():
    from gcc_amd import finetune_main

    base = dict(dataset="imdb-binary", rw_hops=16, subgraph_size=16, restart_prob=0.8, positional_embedding_size=8, batch_size=4,
                seed=0, edge_multiplicity=0, graphs_npz=None)
    with pytest.raises(SystemExit, match="--tu-parse device says where the files of --tudataset are parsed"):
        finetune_main.load_labelled(argparse.Namespace(tudataset=None, tu_parse="device", graph_batcher="auto", **base), "cpu")
    with pytest.raises(SystemExit, match="not with --graph-batcher host"):
        finetune_main.load_labelled(argparse.Namespace(tudataset="d", tu_parse="device", graph_batcher="host", **base), "cpu")
    with pytest.raises(SystemExit, match="--tu-parse 'gpu': host or device"):
        finetune_main.load_labelled(argparse.Namespace(tudataset="d", tu_parse="gpu", graph_batcher="auto", **base), "cpu")


def test_apply_resume_carries_tu_parse():
    from gcc_amd import finetune_main

    line = argparse.Namespace(fold_idx=0, gpu=0, finetune=True, resume="r", cv=False, dataset="imdb-binary", epochs=1, num_workers=0,
                              batch_size=4, edgelist=None, nodelabel=None, tudataset="d", graphs_npz=None, edge_multiplicity=0,
                              no_prefetch=False, graph_batcher="auto", tu_parse="device")
    kept = finetune_main.apply_resume(line, argparse.Namespace(tu_parse="host", hidden_size=64))
    assert kept.tu_parse == "device" and kept.tudataset == "d" and kept.hidden_size == 64
    del line.tu_parse                                               # (a command line from before the flag)
    assert finetune_main.apply_resume(line, argparse.Namespace(hidden_size=64)).tu_parse is None


def test_datasets_take_a_corpus_or_graphs_never_both_or_neither():
    from gcc_amd.datasets import GraphClassificationDataset, GraphClassificationDatasetLabeled

    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)             # noqa: E731
    corpus = dict(node_first=i32(0, 2, 3), row_ptr=i32(0, 1, 2, 2), col_idx=i32(1, 0), seed_local=i32(0, 0), labels=i32(1, 0),
                  sizes=np.array([2, 1]), entries=np.array([2, 0]))
    graphs = [(np.array([0, 1, 2]), np.array([1, 0])), (np.array([0, 0]), np.zeros(0, dtype=np.int64))]
    for cls, extra in ((GraphClassificationDataset, {}), (GraphClassificationDatasetLabeled, dict(labels=[1, 0]))):
        with pytest.raises(ValueError, match="pass graphs=.* or corpus="):
            cls(device="cpu", **extra)
        with pytest.raises(ValueError, match="pass graphs= or corpus=, not both"):
            cls(graphs=graphs, corpus=corpus, device="cpu", **extra)
        with pytest.raises(ValueError, match='batcher="host" needs graphs='):
            cls(corpus=corpus, device="cpu", batcher="host", **extra)
        with pytest.raises(ValueError, match='batcher="device" needs a GPU device'):
            cls(corpus=corpus, device="cpu", **extra)
        assert cls(graphs=graphs, device="cpu", **extra).batcher == "host"       # (as before)
