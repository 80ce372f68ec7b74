"""python -m gcc_amd.tasks.graph_classification --search against the reference's own GraphClassification.svc_classify(x, y,
search=True) (tests/golden/make_graphcls_search_golden.py executed it on the toy embeddings of graphcls_search_reference.npz): the
same accuracy and the same winners through sklearn's GridSearchCV (--device cpu), through the search kernels on the emulator, and
on the GPU."""
import json
import os

import numpy as np
import pytest

from gcc_amd.tasks import graph_classification as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NPZ = os.path.join(GOLDEN, "graphcls_search_reference.npz")
ARGV = ["--dataset", "toy", "--emb-path", NPZ, "--graphs-npz", NPZ, "--search"]
PLAIN = os.path.join(GOLDEN, "graphcls_reference.npz")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "graphcls_search_reference.json")))


def agrees(result, golden):
    assert result["Micro-F1"] == pytest.approx(golden["result"]["Micro-F1"], abs=1e-12)
    assert result["C"] == [float(c) for c in golden["winners"]] and result["folds"] == 10
    assert list(result) == ["Micro-F1", "folds", "iterations", "C"]


def test_cpu_path_prints_the_reference_result_and_winners(golden, capsys):
    result = T.main(ARGV + ["--device", "cpu", "--seed", str(golden["seed"])])
    agrees(result, golden)
    assert result["iterations"] == 0
    assert capsys.readouterr().out.strip().splitlines()[-1] == str(result)


def test_emulator_engine_prints_the_reference_result_and_winners(golden, tmp_path):
    from tests.hipemu.emu_svc import emu_engine

    out = str(tmp_path / "pred.npz")
    result = T.main(ARGV + ["--device", "cpu", "--save-pred", out], engine=emu_engine())
    agrees(result, golden)
    assert result["iterations"] > 0
    z = np.load(out)
    assert z["C_of_fold"].tolist() == result["C"] and z["decision"].shape == (100, 1)
    assert np.array_equal(z["mean_score"], np.array(golden["mean_score"]))


@pytest.mark.gpu
def test_gpu_prints_the_reference_result_and_winners(golden):
    result = T.main(ARGV + ["--device", "cuda:0"])
    agrees(result, golden)
    assert result["iterations"] > 0


def test_search_options(golden):
    with pytest.raises(SystemExit):
        T.main(ARGV + ["--device", "cpu", "--C", "10"])
    for extra in (["--search-C", "1,ten"], ["--search-C", "0,1"], ["--search-cv", "1"]):
        with pytest.raises(SystemExit):
            T.main(ARGV + ["--device", "cpu"] + extra)
    # a grid of one candidate and three inner folds: that candidate wins every fold
    result = T.main(ARGV + ["--device", "cpu", "--search-C", "10", "--search-cv", "3"])
    assert result["C"] == [10.0] * 10


def test_without_the_flag_nothing_changes(capsys):
    """the plain task on graphcls_reference.npz: the line of the reference's SVC(C=100000) run, no "C" key, --C still honoured"""
    want = json.load(open(os.path.join(GOLDEN, "graphcls_reference.json")))["result"]["Micro-F1"]
    argv = ["--dataset", "toy", "--emb-path", PLAIN, "--graphs-npz", PLAIN, "--device", "cpu"]
    result = T.main(argv)
    assert list(result) == ["Micro-F1", "folds", "iterations"] and result["Micro-F1"] == pytest.approx(want, abs=1e-12)
    assert capsys.readouterr().out.strip().splitlines()[-1] == str(result)
    assert T.main(argv + ["--C", "100000"]) == result
    assert T.main(argv + ["--search-C", "1,2", "--search-cv", "4"]) == result      # (the search's options alone do nothing)
