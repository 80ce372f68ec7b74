"""``--model graphwave`` of the two task front doors: the GraphWave baseline of the reference's node classification and similarity
search.  Node classification runs on the ``task`` fixture of tests/golden/make_graphwave_golden.py (nine cliques of 5 joined in a
ring by paths of 6; its generating script asserts that sklearn's classifier on the reference's table scores 1.0 in all ten folds
with every held-out decision value at least 1.0 from zero, so a difference of 1e-6 between two tables cannot move a prediction).
Similarity search runs on toy ``.graph`` / ``.dict`` pairs written from ``multi130d32`` (its repeated edges as weights) and ``n65d8``."""
import numpy as np
import pytest
import torch

from gcc_amd.tasks import node_classification as NC
from gcc_amd.tasks import similarity_search as SS
from tests import graphwave_reference as R

F32 = 2.0 ** -24                                                    # float32 rounding of entries of magnitude at most 1


def path_first(edges):
    """the path 0-1-2-... first, so that a file's ids in order of appearance are the node ids"""
    return sorted(map(tuple, edges), key=lambda e: (e[1] != e[0] + 1, e))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    fx = R.fixture("task")
    root = tmp_path_factory.mktemp("graphwave_task")
    (root / "toy.edgelist").write_text("".join(f"{u} {v}\n" for u, v in path_first(fx["edges"].tolist())))
    (root / "toy.nodelabel").write_text("".join(f"{i} {int(c)}\n" for i, c in enumerate(fx["labels"])))
    return fx, root


def argv(fx, root, *extra):
    return ["--dataset", "toy", "--model", "graphwave", "--hidden-size", str(fx["d"]), "--edgelist", str(root / "toy.edgelist"),
            "--nodelabel", str(root / "toy.nodelabel"), *extra]


def test_cpu_path_reproduces_the_references_table_and_prints_the_result_line(files, capsys):
    fx, root = files
    out = root / "emb.npy"
    result = NC.main(argv(fx, root, "--device", "cpu", "--save-emb", str(out)))
    printed = capsys.readouterr().out
    assert "{'Micro-F1': " in printed and result["Micro-F1"] == 1.0
    table = np.load(out)
    assert table.dtype == np.float32 and table.shape == (fx["n_rows"], fx["d"])
    assert float(np.abs(table.astype(np.float64) - fx["chi"]).max()) <= R.VARIANT_FACTOR * fx["variant_distance"] + F32


def test_graphwave_takes_no_table_no_seed_and_needs_the_graph(files):
    fx, root = files
    for extra in (["--emb-path", "E.npy"], ["--load-path", "CKPT"], ["--prone-seed", "1"]):
        with pytest.raises(SystemExit):
            NC.main(argv(fx, root, "--device", "cpu", *extra))
    with pytest.raises(SystemExit):
        NC.main(["--dataset", "toy", "--model", "graphwave", "--labels-npz", "L.npz"])
    with pytest.raises(SystemExit):
        NC.main(["--dataset", "toy", "--model", "graphwave", "--emb-path", "E.npy", "--labels-npz", "L.npz"])
    bad_width = [x if x != str(fx["d"]) else "6" for x in argv(fx, root, "--device", "cpu")]
    with pytest.raises(SystemExit):
        NC.main(bad_width)
    with pytest.raises(SystemExit):
        NC.main(["--dataset", "toy", "--model", "deepwalk", "--emb-path", "E.npy", "--labels-npz", "L.npz"])


def test_stand_in_engine_sees_the_graph_and_the_width(files):
    fx, root = files
    seen = {}

    class StandIn:
        def embed(self, row_ptr, col_idx, d, **kw):
            seen.update(row_ptr=np.asarray(row_ptr), col_idx=np.asarray(col_idx), d=d, kw=kw)
            return dict(chi32=torch.from_numpy(fx["chi"].astype(np.float32)), status=torch.zeros(1, dtype=torch.int32))

        def check_status(self, res):
            seen["checked"] = True

    result = NC.main(argv(fx, root, "--device", "cpu"), graphwave_engine=StandIn())
    assert np.array_equal(seen["row_ptr"], fx["row_ptr"]) and np.array_equal(seen["col_idx"], fx["col_idx"])
    assert seen["d"] == fx["d"] and seen["kw"] == {} and seen["checked"]
    assert result["Micro-F1"] == 1.0


@pytest.mark.gpu
def test_device_table_gives_the_cpu_paths_predictions(files):
    fx, root = files
    NC.main(argv(fx, root, "--device", "cpu", "--save-pred", str(root / "cpu.npz")))
    result = NC.main(argv(fx, root, "--device", "cuda:0", "--save-pred", str(root / "gpu.npz"), "--save-emb", str(root / "gpu.npy")))
    cpu, gpu = np.load(root / "cpu.npz"), np.load(root / "gpu.npz")
    assert np.array_equal(cpu["pred"], gpu["pred"]) and np.array_equal(cpu["fold"], gpu["fold"])
    assert result["Micro-F1"] == 1.0
    table = np.load(root / "gpu.npy").astype(np.float64)
    assert float(np.abs(table - fx["chi"]).max()) <= R.VARIANT_FACTOR * fx["variant_distance"] + F32


# ---- similarity search

NETWORKS = {"multi": "multi130d32", "small": "n65d8"}
WIDTH = 8


@pytest.fixture(scope="module")
def panther(tmp_path_factory):
    """``multi.graph`` / ``small.graph`` and their dicts: the authors a0..a64 are in both, under their node ids"""
    root = tmp_path_factory.mktemp("graphwave_panther")
    for net, name in NETWORKS.items():
        fx = R.fixture(name)
        pairs, counts = np.unique(fx["edges"], axis=0, return_counts=True)
        weight = {tuple(p): int(c) for p, c in zip(pairs.tolist(), counts)}
        (root / f"{net}.graph").write_text(f"{fx['n_rows']} {len(weight)}\n" +
                                           "".join(f"{u} {v} {weight[(u, v)]}\n" for u, v in path_first(weight)))
        (root / f"{net}.dict").write_text("".join(f"a{i}\t{i}\n" for i in range(fx["n_rows"])))
    return root


def ss_argv(root, *extra):
    return ["--dataset", "multi_small", "--data-root", str(root), "--k", "5", "10", *extra]


def test_similarity_search_cpu_path_stores_the_references_tables(panther, capsys):
    out = panther / "tables"
    result = SS.main(ss_argv(panther, "--model", "graphwave", "--hidden-size", str(WIDTH), "--device", "cpu", "--save-emb", str(out)))
    line = capsys.readouterr().out
    assert result["queries"] == 65 and "Recall @ 5" in line
    for net, name in NETWORKS.items():
        fx = R.fixture(name)
        table = np.load(out / f"{net}.npy")
        assert table.dtype == np.float32 and table.shape == (fx["n_rows"], WIDTH)
        # the time points 0 and 100 of width 8 are the first and the last of every width: the reference's columns for them
        T = fx["d"] // 4
        ref = fx["chi"][:, [i * 2 * T + q for i in range(2) for q in (0, 1, 2 * (T - 1), 2 * (T - 1) + 1)]]
        assert float(np.abs(table.astype(np.float64) - ref).max()) <= R.VARIANT_FACTOR * fx["variant_distance"] + F32
    # the tables that exist: --model from_numpy and no --model print the line the search of these files printed
    paths = ["--emb-path-1", str(out / "multi.npy"), "--emb-path-2", str(out / "small.npy"), "--device", "cpu"]
    lines = []
    for extra in (["--model", "from_numpy"], []):
        assert SS.main(ss_argv(panther, *paths, *extra)) == result
        lines.append(capsys.readouterr().out)
    assert lines[0] == lines[1] == line
    assert SS.main(ss_argv(panther, *paths, "--hidden-size", str(WIDTH))) == result           # (the reference's option: checked)
    with pytest.raises(SystemExit):
        SS.main(ss_argv(panther, *paths, "--hidden-size", "64"))


def test_similarity_search_flags(panther):
    for extra in (["--model", "graphwave", "--load-path", "CKPT"], ["--model", "graphwave", "--emb-path-1", "A.npy"],
                  ["--model", "graphwave", "--hidden-size", "6"], ["--model", "prone"], []):
        with pytest.raises(SystemExit):
            SS.main(ss_argv(panther, "--device", "cpu", *extra))


def test_similarity_search_stand_in_engine_sees_the_multigraph(panther):
    seen = []

    class StandIn:
        def embed(self, row_ptr, col_idx, d, **kw):
            seen.append((np.asarray(row_ptr), np.asarray(col_idx), d, kw))
            table = R.embed_numpy(row_ptr, col_idx, d)["chi32"]
            return dict(chi32=torch.from_numpy(table), status=torch.zeros(1, dtype=torch.int32))

        def check_status(self, res):
            pass

    SS.main(ss_argv(panther, "--model", "graphwave", "--hidden-size", "8", "--device", "cpu"), graphwave_engine=StandIn())
    fx = R.fixture("multi130d32")
    assert len(seen) == 2 and seen[0][2] == 8 and seen[0][3] == {}
    assert np.array_equal(seen[0][0], fx["row_ptr"]) and np.array_equal(seen[0][1], fx["col_idx"])          # (repeated entries kept)


@pytest.mark.gpu
def test_similarity_search_device_line_is_the_cpu_paths(panther, capsys):
    common = ["--model", "graphwave", "--hidden-size", str(WIDTH)]
    cpu = SS.main(ss_argv(panther, *common, "--device", "cpu"))
    cpu_line = capsys.readouterr().out
    gpu = SS.main(ss_argv(panther, *common, "--device", "cuda:0"))
    assert gpu == cpu and capsys.readouterr().out == cpu_line
