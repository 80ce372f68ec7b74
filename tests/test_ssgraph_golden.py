"""The ``<name>.graph`` reader against the reference's own ``SSSingleDataset`` + ``_create_dgl_graph`` + ``__getitem__``, executed
on a toy weighted network by tests/golden/make_ssgraph_golden.py: the multigraph edge for edge, the node indices, and the
out-degree rule of every item."""
import json
import os

import numpy as np
import pytest

from gcc_amd import ingest
from gcc_amd.graphgen import check_contract, check_multigraph_contract

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ssgraph_reference.json")


@pytest.fixture(scope="module")
def ref():
    return json.load(open(GOLD))


@pytest.fixture()
def files(ref, tmp_path):
    (tmp_path / "toy.graph").write_text(ref["graph"])
    (tmp_path / "toy.dict").write_text(ref["dict"])
    return str(tmp_path / "toy.graph"), str(tmp_path / "toy.dict")


def test_reader_reproduces_the_reference_multigraph(ref, files):
    d = ingest.read_ss_graph(*files, csr=True)
    assert d["node2id"] == {int(k): v for k, v in ref["node2id"].items()} and d["name_dict"] == ref["name_dict"]
    n = ref["num_nodes"]
    assert d["num_graph_nodes"] == n == 40 and d["num_nodes"] == n + 1      # one id only the dict knows: no row for it
    rp, ci, mult = d["row_ptr"], d["col_idx"], d["edge_multiplicity"]
    assert mult == 2 and rp.dtype == ci.dtype == np.int32 and len(rp) == n + 1
    check_multigraph_contract(rp, ci)
    with pytest.raises(ValueError, match="duplicate"):
        check_contract(rp, ci)
    # the DGL multigraph, edge for edge: every CSR entry ``edge_multiplicity`` times
    src = np.repeat(np.arange(n), np.diff(rp))
    got = sorted(zip(np.repeat(src, mult).tolist(), np.repeat(ci, mult).tolist()))
    assert got == sorted(map(tuple, ref["dgl_edges"]))
    # and the reader's own edge list (before the double insertion)
    assert sorted(zip(src.tolist(), ci.tolist())) == sorted(zip(*ref["edge_index"]))
    weights = [int(line.split()[2]) for line in ref["graph"].splitlines()[1:]]
    assert sorted(set(weights)) == [1, 2, 3, 4, 5] and len(ci) == 2 * sum(weights)


def test_default_builds_no_csr(files):
    d = ingest.read_ss_graph(*files)
    assert "row_ptr" not in d and "edge_multiplicity" not in d and d["num_nodes"] == 41


def test_dataset_ltab_is_the_reference_out_degree_rule(ref, files):
    from gcc_amd.datasets import NodeClassificationDataset

    d = ingest.read_ss_graph(*files, csr=True)
    ds = NodeClassificationDataset("toy", rw_hops=ref["rw_hops"], restart_prob=ref["restart_prob"], graph=(d["row_ptr"], d["col_idx"]),
                                   edge_multiplicity=d["edge_multiplicity"], batch_size=16, multigraph=True,
                                   sample_fn=lambda first, seeds: None)
    deg = np.diff(d["row_ptr"])
    assert len(ds) == len(ref["items"]) == ref["num_nodes"]
    for item in ref["items"]:
        v = item["idx"]
        assert item["seeds"] == [v, v] and item["out_degree"] == deg[v] * d["edge_multiplicity"]
        assert int(ds.ltab[deg[v]]) == item["max_nodes_per_seed"], item
    assert len({i["max_nodes_per_seed"] for i in ref["items"]}) > 5          # the rule is exercised above the rw_hops floor


def test_multigraph_csr_and_edgelist_flag(tmp_path):
    rp, ci = ingest.multigraph_csr(np.array([[0, 1], [2, 1], [1, 0]]), np.array([2, 1, 3]), 3)
    assert rp.tolist() == [0, 5, 11, 12] and ci.tolist() == [1] * 5 + [0] * 5 + [2] + [1]      # a pair listed twice: weights add
    for pairs, w, match in (([[0, 0]], [1], "self loop"), ([[0, 1]], [0], "positive"), ([[0, 2]], [1], "isolated"),
                            ([[0, 3]], [1], "out of range")):
        with pytest.raises(ValueError, match=match):
            ingest.multigraph_csr(np.array(pairs), np.array(w), 3)
    (tmp_path / "bad.edgelist").write_text("1 2\n2 3\n1 2\n")
    with pytest.raises(ValueError, match="non-uniform"):
        ingest.read_edgelist(str(tmp_path / "bad.edgelist"))                 # the default stays a refusal
    d = ingest.read_edgelist(str(tmp_path / "bad.edgelist"), multigraph=True)
    assert d["multigraph"] and d["edge_multiplicity"] == 2
    assert d["row_ptr"].tolist() == [0, 2, 5, 6] and d["col_idx"].tolist() == [1, 1, 0, 0, 2, 1]
    (tmp_path / "ok.edgelist").write_text("1 2\n2 3\n")
    d = ingest.read_edgelist(str(tmp_path / "ok.edgelist"), multigraph=True)
    assert not d["multigraph"] and d["col_idx"].tolist() == [1, 0, 2, 1]
    (tmp_path / "loop.edgelist").write_text("1 2\n2 2\n1 2\n")
    with pytest.raises(ValueError, match="self loop"):
        ingest.read_edgelist(str(tmp_path / "loop.edgelist"), multigraph=True)
