"""The similarity-search task against the reference's own run (tests/golden/make_similarity_golden.py): the reader of the
``.graph`` / ``.dict`` pairs reproduces ``SSDataset._preprocess`` entry for entry, and the task gives exactly the reference's
Recall@20 / Recall@40 -- on the host path, through the kernels on the emulator, and on the device."""
import json
import os

import numpy as np
import pytest

from gcc_amd.ingest import read_ss_graph
from gcc_amd.tasks.similarity_search import evaluate

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    r = json.load(open(os.path.join(GOLDEN, "similarity_reference.json")))
    z = np.load(os.path.join(GOLDEN, "similarity_reference.npz"))
    r["emb_1"], r["emb_2"] = z["emb_1"], z["emb_2"]
    return r


@pytest.fixture(scope="module")
def networks(ref, tmp_path_factory):
    td = tmp_path_factory.mktemp("panther")
    for fn, text in ref["files"].items():
        (td / fn).write_text(text)
    return {name: read_ss_graph(str(td / (name + ".graph")), str(td / (name + ".dict"))) for name in ("toya", "toyb")}


@pytest.mark.parametrize("name", ["toya", "toyb"])
def test_reader_reproduces_the_reference_preprocess(ref, networks, name):
    got, want = networks[name], ref["preprocess"][name]
    assert {str(k): v for k, v in got["node2id"].items()} == want["node2id"]
    assert list(got["node2id"].values()) == list(range(got["num_nodes"]))          # indices in order of first appearance
    assert got["name_dict"] == want["name_dict"]
    assert got["pairs"].dtype == np.int64 and got["weights"].dtype == np.int64 and len(got["pairs"]) == len(got["weights"])
    # the reference's edge list: every pair `weight` times, each time in both directions
    rep = np.repeat(got["pairs"], got["weights"], axis=0)
    edges = np.stack([rep, rep[:, ::-1]], axis=1).reshape(-1, 2)
    assert edges.T.tolist() == want["edge_index"]
    assert max(want["name_dict"].values()) >= ref["rows"][0 if name == "toya" else 1]   # some keys lie past the table's end


def _check(ref, result):
    assert result["queries"] == ref["queries"]
    for k in (20, 40):
        assert result[f"Recall @ {k}"] == ref["result"][f"Recall @ {k}"]


def test_host_path_gives_the_reference_recall(ref, networks):
    result, detail = evaluate(ref["emb_1"], ref["emb_2"], networks["toya"]["name_dict"], networks["toyb"]["name_dict"],
                              device="cpu", with_topk=True)
    _check(ref, result)
    hit = detail["greater"] + detail["equal_before"] < 40
    assert (hit == (detail["topk_col"] == detail["target"][:, None]).any(1)).all()


def test_kernels_on_the_emulator_give_the_reference_recall(ref, networks):
    from gcc_amd.simsearch import SimilarityEngine
    from tests.hipemu.emu_driver import emu_lib

    engine = SimilarityEngine(emu_lib(), lambda t: t.data_ptr() if t is not None else None)
    result, detail = evaluate(ref["emb_1"], ref["emb_2"], networks["toya"]["name_dict"], networks["toyb"]["name_dict"],
                              device="cpu", with_topk=True, engine=engine)
    _check(ref, result)
    hit = detail["greater"] + detail["equal_before"] < 40
    assert (hit == (detail["topk_col"] == detail["target"][:, None]).any(1)).all()


@pytest.mark.gpu
def test_device_gives_the_reference_recall(ref, networks):
    result, detail = evaluate(ref["emb_1"], ref["emb_2"], networks["toya"]["name_dict"], networks["toyb"]["name_dict"],
                              device="cuda:0", with_topk=True)
    _check(ref, result)
    hit = detail["greater"] + detail["equal_before"] < 40
    assert (hit == (detail["topk_col"] == detail["target"][:, None]).any(1)).all()
