"""python -m gcc_amd.tasks.graph_classification against the reference's own GraphClassification.svc_classify
(tests/golden/make_graphcls_golden.py executed it on the toy embeddings of graphcls_reference.npz): the same accuracy through
sklearn (--device cpu), through the SVC kernels on the emulator, and on the GPU."""
import json
import os

import numpy as np
import pytest

from gcc_amd.tasks import graph_classification as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NPZ = os.path.join(GOLDEN, "graphcls_reference.npz")                  # emb + graph_labels: the table and the corpus' labels
ARGV = ["--dataset", "toy", "--emb-path", NPZ, "--graphs-npz", NPZ]


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "graphcls_reference.json")))


def test_cpu_path_prints_the_reference_result(golden, capsys):
    result = T.main(ARGV + ["--device", "cpu", "--seed", str(golden["seed"]), "--model", "from_numpy_graph", "--hidden-size", "16",
                            "--num-shuffle", "10"])
    assert result["Micro-F1"] == pytest.approx(golden["result"]["Micro-F1"], abs=1e-12)
    assert result["folds"] == 10 and result["iterations"] == 0 and list(result) == ["Micro-F1", "folds", "iterations"]
    assert capsys.readouterr().out.strip().splitlines()[-1] == str(result)


def test_emulator_engine_prints_the_reference_result(golden, tmp_path):
    from tests.hipemu.emu_svc import emu_engine

    out = str(tmp_path / "pred.npz")
    result = T.main(ARGV + ["--device", "cpu", "--save-pred", out], engine=emu_engine())
    assert result["Micro-F1"] == pytest.approx(golden["result"]["Micro-F1"], abs=1e-12)
    assert result["iterations"] > 0
    z = np.load(out)
    y = np.load(NPZ)["graph_labels"]
    assert z["decision"].shape == (len(y), 3) and set(z["pred"].tolist()) <= {1, 2, 3} and np.array_equal(z["labels"], y)
    assert np.mean([(z["pred"][z["fold"] == f] == y[z["fold"] == f]).mean() for f in range(10)]) == pytest.approx(result["Micro-F1"])


@pytest.mark.gpu
def test_gpu_prints_the_reference_result(golden):
    result = T.main(ARGV + ["--device", "cuda:0"])
    assert result["Micro-F1"] == pytest.approx(golden["result"]["Micro-F1"], abs=1e-12) and result["iterations"] > 0


def test_load_path_embeds_the_corpus_first(golden, monkeypatch):
    import torch

    import gcc_amd.generate as G

    seen = {}

    def fake_run(args_test, pipeline=None, save=True):
        seen.update(vars(args_test), save=save)
        return torch.from_numpy(np.load(NPZ)["emb"])

    monkeypatch.setattr(G, "run", fake_run)
    result = T.main(["--dataset", "toy", "--load-path", "ckpt.pth", "--graphs-npz", NPZ, "--device", "cpu", "--batch-size", "32"])
    assert result["Micro-F1"] == pytest.approx(golden["result"]["Micro-F1"], abs=1e-12)
    assert seen["load_path"] == "ckpt.pth" and seen["graphs_npz"] == NPZ and seen["tudataset"] is None and seen["save"] is False
    assert seen["batch_size"] == 32 and seen["gpu"] is None and seen["dataset"] == "toy"


def test_command_line_errors():
    for extra in (["--model", "gin"], ["--hidden-size", "64"], ["--load-path", "x.pth"], ["--tudataset", "somewhere"]):
        with pytest.raises(SystemExit):
            T.main(ARGV + ["--device", "cpu"] + extra)
    with pytest.raises(SystemExit):
        T.main(["--dataset", "toy", "--emb-path", NPZ, "--device", "cpu"])
    with pytest.raises(ValueError, match="embedding rows"):
        T.evaluate(np.zeros((5, 4), np.float32), np.arange(6) % 2)


def test_a_row_without_a_vote_is_stored_as_minus_one():
    """sklearn is not asked (its SVC would raise on a one-class fold): a stand-in engine returns pred -1 for two rows"""
    import torch

    class NoVote:
        def fit_predict_folds(self, x, labels, fold, C):
            pred = torch.from_numpy(np.asarray(labels, dtype=np.int32).copy())
            pred[[3, 7]] = -1
            return dict(pred=pred, decision=torch.zeros(len(labels), 1, dtype=torch.float64), iters=torch.zeros(1, dtype=torch.int32),
                        status=torch.zeros(1, dtype=torch.int32))

        def check_status(self, res, allow_iter_cap=False):
            pass

    y = np.array([5, 9] * 20)
    result, detail = T.evaluate(np.zeros((40, 4), np.float32), y, engine=NoVote())
    assert detail["pred"][3] == -1 and detail["pred"][7] == -1 and np.array_equal(np.delete(detail["pred"], [3, 7]), np.delete(y, [3, 7]))
    assert result["Micro-F1"] == pytest.approx(38 / 40)
