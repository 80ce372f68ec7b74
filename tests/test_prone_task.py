"""``python -m gcc_amd.tasks.node_classification --model prone``: the ProNE baseline of the reference's node classification, on
the ``task`` fixture of tests/golden/make_prone_golden.py (two planted communities of 50 nodes; its generating script asserts
that every row of the reference's embedding is nearer to its own class centroid than to the other's by 0.25 in cosine
similarity, so a difference of 1e-6 between two tables cannot move a prediction)."""
import numpy as np
import pytest
import torch

from gcc_amd.tasks import node_classification as NC
from tests import prone_reference as R


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the fixture's edge list (the path 0-1-2-... comes first, so the file's ids are the node ids) and labels"""
    fx = R.fixture("task")
    root = tmp_path_factory.mktemp("prone_task")
    edges = sorted(map(tuple, fx["edges"].tolist()), key=lambda e: (e[1] != e[0] + 1, e))
    (root / "toy.edgelist").write_text("".join(f"{u} {v}\n" for u, v in edges))
    (root / "toy.nodelabel").write_text("".join(f"{i} {int(c)}\n" for i, c in enumerate(fx["labels"])))
    return fx, root


def argv(fx, root, *extra):
    return ["--dataset", "toy", "--model", "prone", "--hidden-size", str(fx["d"]), "--edgelist", str(root / "toy.edgelist"),
            "--nodelabel", str(root / "toy.nodelabel"), "--prone-seed", str(fx["seed"]), *extra]


def test_cpu_path_reproduces_the_references_embedding_and_prints_the_result_line(files, capsys):
    fx, root = files
    out = root / "emb.npy"
    result = NC.main(argv(fx, root, "--device", "cpu", "--save-emb", str(out), "--save-pred", str(root / "cpu.npz")))
    printed = capsys.readouterr().out
    assert "{'Micro-F1': " in printed and result["Micro-F1"] == 1.0
    table = np.load(out)
    assert table.dtype == np.float32 and table.shape == (fx["n"], fx["d"])
    lu = fx["emb_lu"]
    # float32 rounding of entries below 1 (2^-24) on top of the float64 bound
    assert float(np.abs(R.align(table.astype(np.float64), lu) - lu).max()) <= R.VARIANT_FACTOR * fx["variant_distance"] + 2.0 ** -24


def test_prone_takes_no_table_and_needs_the_graph(files):
    fx, root = files
    for extra in (["--emb-path", "E.npy"], ["--load-path", "CKPT"]):
        with pytest.raises(SystemExit):
            NC.main(argv(fx, root, "--device", "cpu", *extra))
    with pytest.raises(SystemExit):
        NC.main(["--dataset", "toy", "--model", "prone", "--labels-npz", "L.npz"])
    with pytest.raises(SystemExit):
        NC.main(["--dataset", "toy", "--model", "graphwave", "--emb-path", "E.npy", "--labels-npz", "L.npz"])
    with pytest.raises(SystemExit):                                # (--save-emb goes with --model prone alone)
        NC.main(["--dataset", "toy", "--emb-path", "E.npy", "--labels-npz", "L.npz", "--save-emb", "O.npy"])


def test_stand_in_engine_sees_the_graph_the_width_and_the_seed(files):
    fx, root = files
    seen = {}

    class StandIn:
        def embed(self, row_ptr, col_idx, d, seed=0, **kw):
            seen.update(row_ptr=np.asarray(row_ptr), col_idx=np.asarray(col_idx), d=d, seed=seed, kw=kw)
            return dict(emb32=torch.from_numpy(fx["emb_lu"].astype(np.float32)), status=torch.zeros(1, dtype=torch.int32))

        def check_status(self, res):
            seen["checked"] = True

    result = NC.main(argv(fx, root, "--device", "cpu"), prone_engine=StandIn())
    assert np.array_equal(seen["row_ptr"], fx["row_ptr"]) and np.array_equal(seen["col_idx"], fx["col_idx"])
    assert seen["d"] == fx["d"] and seen["seed"] == fx["seed"] and seen["kw"] == {} and seen["checked"]
    assert result["Micro-F1"] == 1.0
    seen.clear()
    plain = [a for a in argv(fx, root) if a not in ("--prone-seed", str(fx["seed"]))]
    NC.main(plain + ["--device", "cpu", "--seed", "3"], prone_engine=StandIn())                  # without --prone-seed: --seed
    assert seen["seed"] == 3


@pytest.mark.gpu
def test_device_table_gives_the_cpu_paths_predictions(files):
    fx, root = files
    NC.main(argv(fx, root, "--device", "cpu", "--save-pred", str(root / "cpu.npz")))
    result = NC.main(argv(fx, root, "--device", "cuda:0", "--save-pred", str(root / "gpu.npz"), "--save-emb", str(root / "gpu.npy")))
    cpu, gpu = np.load(root / "cpu.npz"), np.load(root / "gpu.npz")
    assert np.array_equal(cpu["pred"], gpu["pred"]) and np.array_equal(cpu["fold"], gpu["fold"])
    assert result["Micro-F1"] == 1.0
    lu = fx["emb_lu"]
    table = np.load(root / "gpu.npy").astype(np.float64)
    assert float(np.abs(R.align(table, lu) - lu).max()) <= R.VARIANT_FACTOR * fx["variant_distance"] + 2.0 ** -24
