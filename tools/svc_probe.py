"""Times the ten-fold frozen-embedding protocol (StratifiedKFold(10), an RBF C-SVC with C = 100000 per fold) on the MI355X --
gcc_amd.svc.SVCEngine, all folds and class pairs in one pass -- against sklearn's SVC, fold by fold, on the same host:

    easy    1,000 unit-norm rows of 64 columns, two classes 0.15 apart: a few hundred SMO iterations per fold
    hard    300 unit-norm rows of 2 columns, two overlapping classes: nearly hard-margin, millions of iterations per fold
    large   4,200 unit-norm rows of 64 columns, two classes 0.15 apart: 3,780 rows per problem, the scale of COLLAB's largest pair
    corpus  the embeddings of a TU corpus, when --emb-path with --tudataset / --graphs-npz is given

The device's wall time is taken around fit_predict_folds and includes the one host read per launch; sklearn's is the ten fits
and predictions.  Reported per case: both times, their ratio, the iterations, the launches and whether the two sides predict
the same labels (they stop at the same tolerance but not at the same point, so a row with a decision value near 0 may differ).

    python tools/svc_probe.py [--out profiles/svc_probe.json] [--cases easy hard large] [--emb-path E.npy --dataset NAME --tudataset DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcc_amd.svc import SVCEngine  # noqa: E402
from gcc_amd.tasks import graph_classification as T  # noqa: E402


def synthetic(rows, columns, shift, seed):
    rng = np.random.RandomState(seed)
    y = (np.arange(rows) % 2).astype(np.int64)
    x = rng.randn(rows, columns) + shift * (2 * y[:, None] - 1)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), y


def probe(name, x, y, engine, dev, C, seed=0):
    fold = T.fold_ids(y, seed)
    xd = torch.from_numpy(x).to(dev)
    engine.fit_predict_folds(xd[:64], y[:64], fold[:64] % 2, C=1.0)        # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = engine.fit_predict_folds(xd, y, fold, C=C)
    pred = res["pred"].cpu().numpy()
    t1 = time.perf_counter()
    pred_sk, _, _ = T.classify_sklearn(x, y, fold, C)
    t2 = time.perf_counter()
    acc = lambda p: float(np.mean([(p[fold == f] == y[fold == f]).mean() for f in range(T.FOLDS)]))        # noqa: E731
    row = dict(case=name, rows=int(x.shape[0]), columns=int(x.shape[1]), classes=int(y.max()) + 1, C=C,
               device_s=round(t1 - t0, 4), sklearn_s=round(t2 - t1, 4), sklearn_over_device=round((t2 - t1) / (t1 - t0), 3),
               iterations_total=int(res["iters"].sum()), iterations_max=int(res["iters"].max()), launches=res["launches"],
               largest_problem=int(res["problem_rows"].max()), status=int(res["status"].cpu()[0]),
               accuracy_device=acc(pred), accuracy_sklearn=acc(pred_sk), rows_predicted_differently=int((pred != pred_sk).sum()))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "svc_probe.json"))
    ap.add_argument("--cases", nargs="*", default=["easy", "hard", "large"], choices=["easy", "hard", "large"])
    ap.add_argument("--emb-path", default=None)
    ap.add_argument("--dataset", default=None)
    ap.add_argument("--tudataset", default=None)
    ap.add_argument("--graphs-npz", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    engine = SVCEngine()
    results = []
    if "easy" in a.cases:
        results.append(probe("easy", *synthetic(1000, 64, 0.15, 0), engine, dev, 1e5))
    if "hard" in a.cases:
        results.append(probe("hard", *synthetic(300, 2, 0.3, 1), engine, dev, 1e5))
    if "large" in a.cases:
        results.append(probe("large", *synthetic(4200, 64, 0.15, 2), engine, dev, 1e5))
    if a.emb_path:
        y = np.unique(T.load_labels(a), return_inverse=True)[1]
        x = np.ascontiguousarray(T.load_embedding(a.emb_path), dtype=np.float32)
        results.append(probe(a.dataset or "corpus", x, y, engine, dev, 1e5))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), host_cpus=os.cpu_count(), results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
