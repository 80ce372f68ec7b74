"""Generates tests/golden/graphcls_reference.json and graphcls_reference.npz by EXECUTING THE REFERENCE'S OWN
``GraphClassification.svc_classify`` (gcc/tasks/graph_classification.py:47-64: StratifiedKFold(10, shuffle=True,
random_state=seed), SVC(C=100000) per fold, mean accuracy) on toy embeddings of three classes.  DGL is replaced by dgl_stub and
the modules the reference imports but this path never calls by empty stand-ins.  Stored: the embeddings (float32), the labels
and the printed result -- inputs and outputs only.

The script picks the first seed for which every held-out decision value of sklearn's converged fits is at least 0.02 from
zero, so solvers that agree within the decision tolerance of tests/svc_check.py predict the same labels and the accuracy is
reproduced exactly.
Run from the repo root:  python tests/golden/make_graphcls_golden.py
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import dgl_stub  # noqa: E402

dgl_stub.install()
for absent in ("seaborn", "pygsp", "tqdm", "networkx"):
    try:
        __import__(absent)
    except ImportError:
        m = types.ModuleType(absent)
        m.tqdm = lambda x, *a, **k: x
        sys.modules[absent] = m
sys.path.insert(0, "/root/reference")

from gcc.tasks.graph_classification import GraphClassification  # noqa: E402
from sklearn.model_selection import StratifiedKFold  # noqa: E402
from sklearn.svm import SVC  # noqa: E402

SEED, ROWS, DIM, MARGIN = 0, 120, 16, 0.02


def toy(seed):
    rng = np.random.RandomState(seed)
    y = (np.arange(ROWS) % 3).astype(np.int64) + 1                 # labels 1, 2, 3: re-indexed by the task
    centres = 0.45 * rng.randn(3, DIM)
    x = centres[y - 1] + rng.randn(ROWS, DIM)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), y


def margin(x, y):
    low = np.inf
    for tr, te in StratifiedKFold(n_splits=10, shuffle=True, random_state=SEED).split(x, y):
        clf = SVC(C=100000, tol=1e-7, decision_function_shape="ovo").fit(x[tr], y[tr])
        low = min(low, float(np.abs(clf.decision_function(x[te])).min()))
    return low


def main():
    for data_seed in range(1000):
        x, y = toy(data_seed)
        if margin(x, y) >= MARGIN:
            break
    else:
        raise RuntimeError("no toy corpus with the margin found")
    task = types.SimpleNamespace(seed=SEED)
    res = GraphClassification.svc_classify(task, x, y, False)
    assert 0.4 < res["Micro-F1"] < 0.95, res
    out = dict(seed=SEED, data_seed=data_seed, margin=margin(x, y), result={k: float(v) for k, v in res.items()})
    json.dump(out, open(os.path.join(HERE, "graphcls_reference.json"), "w"))
    np.savez_compressed(os.path.join(HERE, "graphcls_reference.npz"), emb=x, graph_labels=y)
    print(out)


if __name__ == "__main__":
    main()
