"""Times the nested protocol of graph classification with --search -- StratifiedKFold(10), per fold GridSearchCV(SVC(), {"C": [1,
10, 100, 1000, 10000, 100000]}, cv=5) and a refit -- on the MI355X, on tools/svc_probe.py's shapes

    easy    1,000 unit-norm rows of 64 columns, two classes 0.15 apart: 300 inner problems of 720 rows
    large   4,200 unit-norm rows of 64 columns, two classes 0.15 apart: 300 inner problems of 3,024 rows, refits of 3,780

four ways: the device search (SVCEngine.search_fit_predict_folds: every inner problem side by side over one distance matrix); the
60-call composition of the plain engine (fit_predict_folds on every outer fold's training rows with the inner folds as its folds, once
per candidate, then one plain call per distinct winner), in the same process; sklearn's GridSearchCV(n_jobs=16) per outer fold on
the same host; and one plain fit_predict_folds at C = 100000, for scale.  Each figure is the median of five runs, host reads
included.  The phase shares of the device search come from one further run that synchronises after every phase.

    python tools/svc_search_probe.py [--out profiles/svc_search_probe.json] [--cases easy large] [--repeat 5] [--jobs 16]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcc_amd.svc import SVCEngine, inner_fold_table  # noqa: E402
from gcc_amd.tasks import graph_classification as T  # noqa: E402

CS, CV = list(T.SEARCH_C), 5


def synthetic(rows, columns, shift, seed):
    rng = np.random.RandomState(seed)
    y = (np.arange(rows) % 2).astype(np.int64)
    x = rng.randn(rows, columns) + shift * (2 * y[:, None] - 1)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), y


def timed(fn, repeat):
    times, value = [], None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), value


def composition(engine, xd, y, fold, inner):
    """the search from the plain call alone: 60 calls on sub-corpora, then the refits -> (winners, count table)"""
    folds = int(fold.max()) + 1
    correct = np.zeros((folds, len(CS), CV), dtype=np.int64)
    for o in range(folds):
        tr = np.nonzero(fold != o)[0]
        sub, ids = xd[torch.from_numpy(tr).to(xd.device)], inner[o, tr]
        for c, C in enumerate(CS):
            pred = engine.fit_predict_folds(sub, y[tr], ids, C=C, folds=CV)["pred"].cpu().numpy()
            correct[o, c] = [(pred[ids == i] == y[tr][ids == i]).sum() for i in range(CV)]
    sizes = np.stack([np.bincount(inner[o, fold != o], minlength=CV) for o in range(folds)])
    winners = np.asarray(CS)[np.argmax(np.mean(correct / sizes[:, None, :], axis=-1), axis=1)]
    pred = np.full(len(y), -1)
    for C in sorted(set(winners.tolist())):
        p = engine.fit_predict_folds(xd, y, fold, C=C)["pred"].cpu().numpy()
        take = np.isin(fold, np.nonzero(winners == C)[0])
        pred[take] = p[take]
    return winners, correct, pred


def sklearn_search(x, y, fold, jobs):
    from sklearn.model_selection import GridSearchCV
    from sklearn.svm import SVC

    winners, pred = [], np.full(len(y), -1)
    for f in range(int(fold.max()) + 1):
        tr, te = fold != f, fold == f
        grid = GridSearchCV(SVC(), {"C": CS}, cv=CV, scoring="accuracy", n_jobs=jobs).fit(x[tr], y[tr])
        winners.append(float(grid.best_params_["C"]))
        pred[te] = grid.predict(x[te])
    return np.asarray(winners), pred


def probe(name, x, y, engine, dev, repeat, jobs, seed=0):
    fold = T.fold_ids(y, seed)
    inner = inner_fold_table(y, fold, CV)
    xd = torch.from_numpy(x).to(dev)
    engine.search_fit_predict_folds(xd[:64], y[:64], fold[:64] % 2, inner_fold_table(y[:64], fold[:64] % 2, 2), CS[:2])   # warm-up
    engine.fit_predict_folds(xd[:64], y[:64], fold[:64] % 2, C=1.0)
    acc = lambda p: float(np.mean([(p[fold == f] == y[fold == f]).mean() for f in range(T.FOLDS)]))        # noqa: E731

    def device():
        res = engine.search_fit_predict_folds(xd, y, fold, inner, CS)
        res["pred_h"] = res["pred"].cpu().numpy()
        return res

    t_dev, res = timed(device, repeat)
    t_comp, (w_comp, correct_comp, pred_comp) = timed(lambda: composition(engine, xd, y, fold, inner), repeat)
    t_plain, _ = timed(lambda: engine.fit_predict_folds(xd, y, fold, C=1e5)["pred"].cpu(), repeat)
    t_sk, (w_sk, pred_sk) = timed(lambda: sklearn_search(x, y, fold, jobs), repeat)
    phases = engine.search_fit_predict_folds(xd, y, fold, inner, CS, profile=True)["phase_s"]
    whole = sum(phases.values())
    iters = res["search_iters"].cpu().numpy()
    row = dict(case=name, rows=int(x.shape[0]), columns=int(x.shape[1]), classes=int(y.max()) + 1, candidates=CS, inner_folds=CV,
               repeat=repeat, inner_problems=int(iters.size), largest_inner_problem=int(res["search_problem_rows"].max()),
               largest_refit_problem=int(res["problem_rows"].max()),
               device_search_s=round(t_dev, 4), composition_s=round(t_comp, 4), sklearn_grid_s=round(t_sk, 4), sklearn_jobs=jobs,
               plain_fit_s=round(t_plain, 4), composition_over_search=round(t_comp / t_dev, 3),
               sklearn_over_search=round(t_sk / t_dev, 3), search_over_plain_fit=round(t_dev / t_plain, 3),
               phase_s={k: round(v, 4) for k, v in phases.items()}, phase_share={k: round(v / whole, 3) for k, v in phases.items()},
               search_iterations_total=int(iters.sum()), search_iterations_max=int(iters.max()),
               refit_iterations_total=int(res["iters"].sum()), search_launches=res["search_launches"], refit_launches=res["launches"],
               status=int(res["status"].cpu()[0]), search_status=int(res["search_status"].cpu()[0]),
               winners_device=res["C_of_fold"].tolist(), winners_sklearn=w_sk.tolist(),
               composition_agrees=bool(np.array_equal(w_comp, res["C_of_fold"]) and np.array_equal(correct_comp, res["correct"])
                                       and np.array_equal(pred_comp, res["pred_h"])),
               accuracy_device=acc(res["pred_h"]), accuracy_sklearn=acc(pred_sk),
               rows_predicted_differently=int((res["pred_h"] != pred_sk).sum()))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "svc_search_probe.json"))
    ap.add_argument("--cases", nargs="*", default=["easy", "large"], choices=["easy", "large"])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=16)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    engine = SVCEngine()
    results = []
    if "easy" in a.cases:
        results.append(probe("easy", *synthetic(1000, 64, 0.15, 0), engine, dev, a.repeat, a.jobs))
    if "large" in a.cases:
        results.append(probe("large", *synthetic(4200, 64, 0.15, 2), engine, dev, a.repeat, a.jobs))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), host_cpus=os.cpu_count(), results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
