"""Generates tests/golden/ssgraph_reference.json by EXECUTING THE REFERENCE'S OWN ``data_util.SSSingleDataset`` (the
``<name>.graph`` reader of the similarity-search networks, data_util.py:111-143), ``NodeClassificationDataset._create_dgl_graph``
(graph_dataset.py:300-308) and ``GraphDataset.__getitem__`` (graph_dataset.py:230-275) on a toy weighted co-author network:
40 authors, weights 1..5 (a pair of weight t is t parallel edges, in both directions by the reader and both again by
``_create_dgl_graph``), one author id that only the ``.dict`` file knows.  ``dgl.DGLGraph`` is a recorder of ``add_nodes`` /
``add_edges`` and ``random_walk_with_restart`` a recorder of what is asked of DGL (seeds, restart_prob, max_nodes_per_seed:
the out-degree rule on the multigraph).  Stored: the file texts, the directed multigraph edge for edge, ``SSDataset``'s name
dict and node2id for the same files, and every item's call.  Fixtures only.
Run from the repo root:  python tests/golden/make_ssgraph_golden.py
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import dgl_stub  # noqa: E402

dgl_stub.install()
dgl = sys.modules["dgl"]
backend = types.ModuleType("dgl.backend")
backend.asnumpy = lambda t: t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
sys.modules["dgl.backend"] = backend
dgl.backend = backend
calls = []


def rwr(g, seeds, restart_prob, max_nodes_per_seed):
    calls.append(dict(seeds=[int(s) for s in seeds], restart_prob=float(restart_prob), max_nodes_per_seed=int(max_nodes_per_seed)))
    return [[torch.tensor([g.nbr(int(s))])] for s in seeds]        # one trace per seed: a single step to a neighbour


sampling = types.ModuleType("dgl.contrib.sampling")
sampling.random_walk_with_restart = rwr
contrib = types.ModuleType("dgl.contrib")
contrib.sampling = sampling
sys.modules["dgl.contrib"], sys.modules["dgl.contrib.sampling"] = contrib, sampling
dgl.contrib = contrib
sys.path.insert(0, "/root/reference")

from make_posemb_golden import StubGraph  # noqa: E402


class RecordingGraph:
    """dgl.DGLGraph as far as _create_dgl_graph and __getitem__ use it: records nodes and edges, answers degrees from them"""

    def __init__(self):
        self.num_nodes, self.edges, self.is_readonly = 0, [], False

    def add_nodes(self, n):
        self.num_nodes += int(n)

    def add_edges(self, src, dst):
        self.edges += list(zip([int(s) for s in src], [int(d) for d in dst]))

    def readonly(self):
        self.is_readonly = True

    def number_of_nodes(self):
        return self.num_nodes

    def out_degree(self, v):
        return sum(1 for s, _ in self.edges if s == v)

    def nbr(self, v):
        return next(d for s, d in self.edges if s == v)

    def subgraph(self, nodes):
        assert len(nodes) == 2
        return StubGraph([0, 1, 2], [1, 0])                  # seed - neighbour


dgl.DGLGraph = RecordingGraph

from gcc.datasets import data_util, graph_dataset  # noqa: E402

RW_HOPS, RESTART = 24, 0.8


def toy_texts():
    rng = np.random.RandomState(8)
    n, extra = 40, 50
    ids = rng.permutation(900)[:n + 1] + 3                   # the last id appears in the dict only
    pairs = {(i, i + 1) for i in range(n - 1)}
    while len(pairs) < n - 1 + extra:
        a, b = sorted(rng.randint(0, n, 2))
        if a != b:
            pairs.add((a, b))
    pairs = sorted(pairs)
    rng.shuffle(pairs)                                       # first appearance is not sorted order
    lines = []
    for a, b in pairs:
        if rng.rand() < 0.5:
            a, b = b, a
        lines.append(f"{ids[a]} {ids[b]} {rng.randint(1, 6)}")
    graph = f"{n} {len(pairs)}\n" + "\n".join(lines) + "\n"
    order = rng.permutation(n + 1)
    names = "".join(f"Author {i}\t{ids[i]}\n" for i in order)
    return graph, names


def main():
    graph_text, dict_text = toy_texts()
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "toy.graph"), "w").write(graph_text)
        open(os.path.join(td, "toy.dict"), "w").write(dict_text)
        single = data_util.SSSingleDataset(td, "toy")
        _, name_dict, node2id = data_util.SSDataset._preprocess(None, td, "toy")
    data = single.get(0)
    g = graph_dataset.NodeClassificationDataset._create_dgl_graph(None, data)
    assert g.is_readonly
    ds = object.__new__(graph_dataset.NodeClassificationDataset)
    ds.graphs = [g]
    ds.step_dist = [1.0, 0.0, 0.0]
    ds.rw_hops, ds.restart_prob = RW_HOPS, RESTART
    ds.positional_embedding_size = 32
    ds.length = ds.total = g.number_of_nodes()
    items = []
    for idx in range(len(ds)):
        calls.clear()
        np.random.seed(idx)
        ds[idx]
        assert len(calls) == 1
        items.append(dict(idx=idx, out_degree=g.out_degree(idx), **calls[0]))
    out = dict(graph=graph_text, dict=dict_text, rw_hops=RW_HOPS, restart_prob=RESTART, edge_index=data.edge_index.tolist(),
               num_nodes=int(g.num_nodes), dgl_edges=g.edges, name_dict={k: int(v) for k, v in name_dict.items()},
               node2id={str(k): int(v) for k, v in node2id.items()}, items=items)
    json.dump(out, open(os.path.join(HERE, "ssgraph_reference.json"), "w"))
    print("nodes", g.num_nodes, "ids", len(node2id), "edge_index columns", data.edge_index.shape[1], "DGL edges", len(g.edges),
          "max_nodes_per_seed", min(i["max_nodes_per_seed"] for i in items), "..", max(i["max_nodes_per_seed"] for i in items))


if __name__ == "__main__":
    main()
