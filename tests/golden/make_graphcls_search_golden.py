"""Generates tests/golden/graphcls_search_reference.json and graphcls_search_reference.npz by EXECUTING THE REFERENCE'S OWN
``GraphClassification.svc_classify(x, y, search=True)`` (gcc/tasks/graph_classification.py:47-64: StratifiedKFold(10,
shuffle=True, random_state=seed), per fold GridSearchCV(SVC(), {"C": [1, 10, 100, 1000, 10000, 100000]}, cv=5,
scoring="accuracy") and its refit, mean accuracy) on toy embeddings of two classes.  DGL is replaced by dgl_stub and the modules the
reference imports but this path never calls by empty stand-ins.  Stored: the embeddings (float32), the labels and the printed
result -- inputs and outputs only -- and, from a restatement of the same protocol with sklearn next to it, the winner of every fold
and the mean-score table (``GridSearchCV.cv_results_``) and the total of ``SVC.n_iter_`` over the inner fits and the refits.

Fixture rule (a condition, not a measurement): the first data seed for which
  * no voting decision value of sklearn's converged fits (tol = 1e-7) lies within tau = max(4 * gap, 1e-4) of zero, over every inner
    and outer held-out row of every candidate; gap = the largest |default - converged| decision difference (tests/svc_check.py's
    rule),
  * sklearn's default and converged fits predict the same labels there, and
  * at least two different winners occur over the ten folds.
On such a corpus a solver within the decision tolerance reproduces winners, count table and accuracy exactly.
Run from the repo root:  python tests/golden/make_graphcls_search_golden.py
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
from sklearn.model_selection import GridSearchCV, StratifiedKFold  # noqa: E402
from sklearn.svm import SVC  # noqa: E402

SEED, ROWS, DIM, SCALE = 0, 100, 16, 0.6
CS, CV = [1, 10, 100, 1000, 10000, 100000], 5


def toy(seed):
    rng = np.random.RandomState(seed)
    y = (np.arange(ROWS) % 2).astype(np.int64) + 1                 # labels 1, 2: re-indexed by the task
    centres = SCALE * rng.randn(2, DIM)
    x = centres[y - 1] + rng.randn(ROWS, DIM)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), y


def survey(x, y):
    """the protocol restated: -> dict(winners, mean_score, n_iter, gap, lowest |converged decision|, same_labels)"""
    gap, low, same, n_iter, winners, table = 0.0, np.inf, True, 0, [], []

    def pair(xtr, ytr, xte, C):
        nonlocal gap, low, same
        sk, conv = SVC(C=C).fit(xtr, ytr), SVC(C=C, tol=1e-7).fit(xtr, ytr)
        d, dc = sk.decision_function(xte), conv.decision_function(xte)
        gap, low = max(gap, float(np.abs(d - dc).max())), min(low, float(np.abs(dc).min()))
        same = same and np.array_equal(sk.predict(xte), conv.predict(xte))
        return int(np.sum(sk.n_iter_))

    for tr, te in StratifiedKFold(n_splits=10, shuffle=True, random_state=SEED).split(x, y):
        grid = GridSearchCV(SVC(), {"C": CS}, cv=CV, scoring="accuracy").fit(x[tr], y[tr])
        winners.append(grid.best_params_["C"])
        table.append([float(v) for v in grid.cv_results_["mean_test_score"]])
        for C in CS:
            refit = pair(x[tr], y[tr], x[te], C)
            n_iter += refit if C == winners[-1] else 0
            for itr, ite in StratifiedKFold(n_splits=CV).split(x[tr], y[tr]):
                n_iter += pair(x[tr][itr], y[tr][itr], x[tr][ite], C)
    return dict(winners=winners, mean_score=table, n_iter=n_iter, gap=gap, low=low, same_labels=bool(same))


def main():
    tried = []
    for data_seed in range(1000):
        x, y = toy(data_seed)
        s = survey(x, y)
        tau = max(4.0 * s["gap"], 1e-4)
        tried.append(dict(data_seed=data_seed, low=s["low"], tau=tau, same_labels=s["same_labels"], winners=sorted(set(s["winners"]))))
        print(tried[-1])
        if s["low"] > tau and s["same_labels"] and len(set(s["winners"])) >= 2:
            break
    else:
        raise RuntimeError("no toy corpus that meets the fixture rule found")
    task = types.SimpleNamespace(seed=SEED)
    res = GraphClassification.svc_classify(task, x, y, True)
    assert 0.4 < res["Micro-F1"] < 0.98, res
    out = dict(seed=SEED, data_seed=data_seed, Cs=CS, cv=CV, result={k: float(v) for k, v in res.items()}, winners=s["winners"],
               mean_score=s["mean_score"], total_n_iter=s["n_iter"], gap=s["gap"], tau=tau, lowest_decision=s["low"], tried=tried)
    json.dump(out, open(os.path.join(HERE, "graphcls_search_reference.json"), "w"))
    np.savez_compressed(os.path.join(HERE, "graphcls_search_reference.npz"), emb=x, graph_labels=y)
    print(out)


if __name__ == "__main__":
    main()
