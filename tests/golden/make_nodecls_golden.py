"""Generates tests/golden/nodecls_reference.json and nodecls_reference.npz by EXECUTING THE REFERENCE'S OWN
``NodeClassification._evaluate`` (gcc/tasks/node_classification.py:53-101: StratifiedKFold(10, shuffle=True, random_state=seed)
over label_matrix.argmax(1), TopKRanker(LogisticRegression(C=1000)) per fold, micro-F1, the mean) on toy embeddings of four
classes, some rows with two labels and one row without any.  DGL is replaced by dgl_stub and the modules the reference imports
but this path never calls by empty stand-ins.  Stored: the embeddings (float32), the label matrix and the printed result --
inputs and outputs only.

The script picks the first data seed for which the reference's printed result (sklearn's default, unconverged fit) equals the
result of the converged fit and every top-k cut of the converged fit is at least 0.02 wide, so solvers that agree within the
decision tolerance of tests/logreg_check.py predict the same label sets and the result is reproduced exactly.
Run from the repo root:  python tests/golden/make_nodecls_golden.py
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

import torch  # noqa: E402
from gcc.tasks.node_classification import NodeClassification, TopKRanker  # noqa: E402
from sklearn.linear_model import LogisticRegression  # noqa: E402
from sklearn.metrics import f1_score  # noqa: E402
from sklearn.model_selection import StratifiedKFold  # noqa: E402

SEED, ROWS, DIM, CLASSES, MARGIN = 0, 240, 16, 4, 0.02


def toy(seed):
    rng = np.random.RandomState(seed)
    cls = np.arange(ROWS) % CLASSES
    x = rng.randn(ROWS, DIM) + 0.6 * rng.randn(CLASSES, DIM)[cls]
    y = np.eye(CLASSES, dtype=np.float32)[cls]
    second = rng.rand(ROWS) < 0.15
    y[np.nonzero(second)[0], (cls[second] + 1) % CLASSES] = 1       # rows with two labels
    y[5] = 0                                                        # a row without labels: k = 0
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), y


def converged(x, y):
    """-> (the mean micro-F1 of the converged fit, its narrowest top-k cut)"""
    scores, low = [], np.inf
    x = x.astype(np.float64)
    for tr, te in StratifiedKFold(n_splits=10, shuffle=True, random_state=SEED).split(x, y.argmax(1)):
        clf = TopKRanker(LogisticRegression(C=1000, solver="newton-cholesky", tol=1e-12, max_iter=1000)).fit(x[tr], y[tr])
        ks = y[te].sum(1).astype(int).tolist()
        scores.append(f1_score(y[te], clf.predict(x[te], ks), average="micro"))
        dec = -np.sort(-clf.decision_function(x[te]), axis=1)
        for r, k in enumerate(ks):
            if 0 < k < CLASSES:
                low = min(low, float(dec[r, k - 1] - dec[r, k]))
    return sum(scores) / len(scores), low


def main():
    for data_seed in range(1000):
        x, y = toy(data_seed)
        res = NodeClassification._evaluate(types.SimpleNamespace(seed=SEED), x.astype(np.float64), torch.Tensor(y), 10)
        score, low = converged(x, y)
        if low >= MARGIN and abs(res["Micro-F1"] - score) <= 1e-12:
            break
    else:
        raise RuntimeError("no toy corpus with the margin found")
    assert 0.4 < res["Micro-F1"] < 0.98, res
    out = dict(seed=SEED, data_seed=data_seed, margin=low, result={k: float(v) for k, v in res.items()})
    json.dump(out, open(os.path.join(HERE, "nodecls_reference.json"), "w"))
    np.savez_compressed(os.path.join(HERE, "nodecls_reference.npz"), emb=x, y=y)
    print(out)


if __name__ == "__main__":
    main()
