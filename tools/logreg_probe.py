"""Times the ten-fold frozen-embedding node-classification protocol (StratifiedKFold(10), one-vs-rest LogisticRegression(C=1000)
per fold, top-k, micro-F1) on the MI355X -- gcc_amd.logreg.LogRegEngine, all folds and classes in one pass, host reads included
-- against sklearn's one-vs-rest fit, fold by fold, on the same host:

    airport  1,190 unit-norm rows of 64 columns, 4 classes: usa_airport's shape
    hindex   5,000 unit-norm rows of 64 columns, 2 classes: h-index's shape
    large    16,384 unit-norm rows of 256 columns, 16 classes

The two sides do not compute the same thing: the device runs Newton's method to the minimiser (max|g| / C <= 1e-9), sklearn its
default lbfgs (tol 1e-4, at most 100 iterations), which is what the reference runs and which stops short of the minimiser.  The
device's wall time is taken around fit_predict_folds plus the copy of the counts to the host; sklearn's is the ten fits, the
probabilities and the ranking.  Per case: a warm-up call, then ``--repeats`` timed calls on the device (median, fastest, slowest)
and ``--sklearn-repeats`` on the host; the Newton iterations, the host reads and the micro-F1 of both sides.

    python tools/logreg_probe.py [--out profiles/logreg_probe.json] [--cases airport hindex large] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcc_amd.logreg import LogRegEngine  # noqa: E402
from gcc_amd.tasks import node_classification as T  # noqa: E402

CASES = {"airport": (1190, 64, 4, 0), "hindex": (5000, 64, 2, 1), "large": (16384, 256, 16, 2)}      # rows, columns, classes, seed


def synthetic(rows, columns, classes, seed):
    """unit-norm rows around one centre per class, one label per row and a second one on 15 % of them"""
    rng = np.random.RandomState(seed)
    cls = np.arange(rows) % classes
    x = rng.randn(rows, columns) + 0.3 * rng.randn(classes, columns)[cls]
    y = np.eye(classes, dtype=np.float32)[cls]
    second = rng.rand(rows) < 0.15
    y[np.nonzero(second)[0], (cls[second] + 1) % classes] = 1
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), y


def spread(times):
    return dict(median=round(statistics.median(times), 4), fastest=round(min(times), 4), slowest=round(max(times), 4), runs=len(times))


def probe(name, x, y, engine, dev, repeats, sklearn_repeats, seed=0):
    fold = T.fold_ids(y.argmax(1), seed)
    xd = torch.from_numpy(x).to(dev)
    engine.fit_predict_folds(xd, y, fold)                              # warm-up: code objects, allocator, the workspace
    torch.cuda.synchronize()
    dev_times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = engine.fit_predict_folds(xd, y, fold)
        counts = res["counts"].cpu().numpy()
        dev_times.append(time.perf_counter() - t0)
    sk_times = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(sklearn_repeats):
            t0 = time.perf_counter()
            _, _, counts_sk, _ = T.classify_sklearn(x, y, fold, 1000.0, "lbfgs")
            sk_times.append(time.perf_counter() - t0)
    f1 = lambda c: float(np.mean([T.fold_f1(*(int(v) for v in c[f])) for f in range(T.FOLDS)]))        # noqa: E731
    d, s = spread(dev_times), spread(sk_times)
    row = dict(case=name, rows=int(x.shape[0]), columns=int(x.shape[1]), classes=int(y.shape[1]), device_s=d, sklearn_s=s,
               sklearn_over_device=round(s["median"] / d["median"], 3), iterations_total=int(res["iters"].sum()),
               iterations_max=int(res["iters"].max()), syncs=res["syncs"], status=int(res["status"].cpu()[0]),
               grad_max=float(res["grad"].max()), micro_f1_device=f1(counts), micro_f1_sklearn_default=f1(counts_sk))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "logreg_probe.json"))
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=list(CASES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sklearn-repeats", type=int, default=3, help="the large case runs sklearn once")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    engine = LogRegEngine()
    results = []
    for name in a.cases:
        rows, columns, classes, seed = CASES[name]
        x, y = synthetic(rows, columns, classes, seed)
        results.append(probe(name, x, y, engine, dev, a.repeats, 1 if name == "large" else a.sklearn_repeats))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), host_cpus=len(os.sched_getaffinity(0)), results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
