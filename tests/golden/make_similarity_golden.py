"""Generates tests/golden/similarity_reference.json and similarity_reference.npz by EXECUTING THE REFERENCE'S OWN
``SSDataset._preprocess`` (data_util.py:159-191) on two toy ``.graph`` / ``.dict`` pairs and ``SimilaritySearch._evaluate``
(gcc/tasks/similarity_search.py:41-69) on two embedding tables with planted, noisy matches.  DGL is replaced by dgl_stub and
the plotting modules the reference imports but this path never calls (seaborn, pygsp) by empty stand-ins.  Stored: the files'
text, the reader's outputs, the tables (float32) and the two recall values -- inputs and outputs only.

Some dict ids appear in no edge (they get fresh indices) and some indices lie past the tables' ends (the key filter drops
them).  The script asserts that every query's hit at 20 and at 40 is the same when its match's float64 score moves by
+-4e-5, so an f32 search must reproduce the two values exactly.
Run from the repo root:  python tests/golden/make_similarity_golden.py
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import dgl_stub  # noqa: E402

dgl_stub.install()
for absent in ("seaborn", "pygsp"):
    sys.modules.setdefault(absent, types.ModuleType(absent))
sys.path.insert(0, "/root/reference")

from gcc.datasets.data_util import SSDataset  # noqa: E402
from gcc.tasks.similarity_search import SimilaritySearch  # noqa: E402

SEED, DIM, ROWS = 0, 32, (400, 450)
DELTA = 4e-5


def toy_network(rng, nodes, edges, listed, prefix, shared):
    """(graph text, dict text): ``nodes`` ids in edges, ``listed`` dict lines of which the last ones name ids no edge has"""
    ids = rng.permutation(100000)[:listed] + 3
    lines = [f"{nodes} {edges}"]
    for _ in range(edges):
        a, b = rng.randint(0, nodes, 2)
        if a != b:
            lines.append(f"{ids[a]} {ids[b]} {rng.randint(1, 4)}")
    names = list(shared) + [f"{prefix} only {i}" for i in range(listed - len(shared))]
    order = rng.permutation(listed)
    dict_text = "".join(f"{names[i]}\t{ids[order[i]]}\n" for i in range(listed))
    return "\n".join(lines) + "\n", dict_text


def main():
    rng = np.random.RandomState(SEED)
    shared = [f"Author {i:03d}" for i in range(260)]
    texts = {}
    for name, nodes, edges, listed in (("toya", 380, 900, 430), ("toyb", 420, 1000, 480)):
        texts[name + ".graph"], texts[name + ".dict"] = toy_network(rng, nodes, edges, listed, name, shared)
    pre = {}
    with tempfile.TemporaryDirectory() as td:
        for fn, text in texts.items():
            open(os.path.join(td, fn), "w").write(text)
        for name in ("toya", "toyb"):
            edge_index, name_dict, node2id = SSDataset._preprocess(None, td, name)
            pre[name] = dict(edge_index=edge_index.tolist(), name_dict={k: int(v) for k, v in name_dict.items()},
                             node2id={str(k): int(v) for k, v in node2id.items()})
    d1, d2 = pre["toya"]["name_dict"], pre["toyb"]["name_dict"]
    emb_1 = rng.randn(ROWS[0], DIM).astype(np.float32)
    emb_2 = rng.randn(ROWS[1], DIM).astype(np.float32)
    for key in shared:                                            # planted matches: the same author, noisily
        if d1[key] < ROWS[0] and d2[key] < ROWS[1]:
            emb_2[d2[key]] = emb_1[d1[key]] + rng.uniform(1.5, 4.5) * rng.randn(DIM).astype(np.float32)
    res = SimilaritySearch._evaluate(None, emb_1.astype(np.float64), emb_2.astype(np.float64), d1, d2)
    # margin: every hit decision in float64 is the same with the match's score moved by +-DELTA
    keys = [x for x in set(d1) & set(d2) if d1[x] < ROWS[0] and d2[x] < ROWS[1]]
    q = emb_1[[d1[x] for x in keys]].astype(np.float64)
    c = emb_2[[d2[x] for x in keys]].astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    s = q @ c.T
    st = np.diag(s)[:, None]
    off = ~np.eye(len(keys), dtype=bool)
    lo, hi = ((s > st + DELTA) & off).sum(1), ((s > st - DELTA) & off).sum(1)
    for k in (20, 40):
        assert ((lo < k) == (hi < k)).all(), f"a hit at {k} is within {DELTA} of flipping: pick another seed"
        assert abs((hi < k).mean() - res[f"Recall @ {k}"]) < 1e-12, "the restatement disagrees with the reference"
    assert 0.1 < res["Recall @ 20"] < res["Recall @ 40"] < 0.9
    out = dict(files=texts, preprocess=pre, rows=list(ROWS), queries=len(keys), result=res)
    json.dump(out, open(os.path.join(HERE, "similarity_reference.json"), "w"))
    np.savez_compressed(os.path.join(HERE, "similarity_reference.npz"), emb_1=emb_1, emb_2=emb_2)
    print(len(keys), "queries", res)


if __name__ == "__main__":
    main()
