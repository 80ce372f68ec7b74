"""Graph classification on frozen embeddings (gcc/tasks/graph_classification.py of the reference, the "GCC (freeze)" column of
the paper's graph-classification table): ``StratifiedKFold(10, shuffle=True, random_state=seed)`` over the graphs' labels, an
RBF C-SVC with C = 100000 per fold, the mean accuracy as ``{"Micro-F1": ...}``.

    python -m gcc_amd.tasks.graph_classification --dataset imdb-binary --emb-path E.npy (--tudataset DIR | --graphs-npz F) \\
        [--seed 0] [--device cuda:0|cpu] [--C 100000 | --search [--search-C 1,10,...] [--search-cv 5]] [--save-pred OUT.npz]
    python -m gcc_amd.tasks.graph_classification --dataset imdb-binary --load-path CKPT (--tudataset DIR | --graphs-npz F) ...

With ``--load-path`` the table need not exist: the corpus is embedded on the device with the checkpoint (what ``generate.py
--tudataset / --graphs-npz`` does) and handed on without a trip through disk.  The labels come from the corpus
(gcc_amd.ingest.read_tudataset, or ``graph_labels`` of the npz).  On a GPU all ten folds and all class pairs are solved in
one pass of gcc_amd.svc.SVCEngine (gcc_amd/csrc/svc.hip); ``--device cpu`` runs sklearn's ``SVC`` itself, fold by fold, as the
reference does.  ``--model from_numpy_graph --hidden-size --num-shuffle`` of the reference's command line are accepted and
checked, nothing more.  Prints the reference's result line with the fold count and the SMO iterations added;
``--save-pred`` stores the predicted label (-1 where no class pair of the fold could vote), the fold and the decision values of
every graph.

``--search`` is the reference's ``svc_classify(x, y, search=True)``: per outer fold ``GridSearchCV(SVC(), {"C": [1, 10, 100,
1000, 10000, 100000]}, cv=5, scoring="accuracy")`` and a refit at the winning C.  On a GPU the 10 x 5 x 6 x pairs inner problems
are solved side by side over the one distance matrix (``SVCEngine.search_fit_predict_folds``); ``--device cpu`` runs sklearn's
``GridSearchCV`` itself.  The result line then carries ``"C"``, the winner of every fold, and ``--save-pred`` also stores
``C_of_fold`` and ``mean_score`` [folds, candidates]."""
from __future__ import annotations

import argparse

import numpy as np

from ._common import FOLDS, checkpoint_table, fold_ids, load_embedding  # noqa: F401  (fold_ids, load_embedding: importable from here)


def classify_sklearn(emb, labels, fold, C):
    """graph_classification.py:47-64 with the folds given: sklearn's SVC per fold -> (pred int32 [N], None, 0)"""
    from sklearn.svm import SVC

    pred = np.full(len(labels), -1, dtype=np.int32)
    for f in range(int(fold.max()) + 1):
        train, test = fold != f, fold == f
        pred[test] = SVC(C=C).fit(emb[train], labels[train]).predict(emb[test])
    return pred, None, 0


def classify_device(emb, labels, fold, C, device, engine=None):
    """-> (pred int32 [N], decision float64 [N, pairs], total SMO iterations)"""
    import torch

    from .. import _cabi
    from ..svc import SVCEngine

    engine = engine if engine is not None else SVCEngine()
    x = torch.from_numpy(np.ascontiguousarray(emb, dtype=np.float32)).to(torch.device(device))
    res = engine.fit_predict_folds(x, labels, fold, C=C)
    engine.check_status(res, allow_iter_cap=True)
    if int(res["status"].cpu()[0]) & _cabi.STATUS_SVC_ITER_CAP:  # libsvm warns and goes on with the solver's state at the cap
        print("warning: a (fold, class pair) problem stopped at the iteration cap before tol was reached")
    return res["pred"].cpu().numpy(), res["decision"].cpu().numpy(), int(res["iters"].sum())


SEARCH_C = (1.0, 10.0, 100.0, 1000.0, 10000.0, 100000.0)          # the reference's grid


def search_sklearn(emb, labels, fold, Cs, cv):
    """graph_classification.py:47-64 with search=True and the folds given: sklearn's GridSearchCV per fold -> (pred int32 [N],
    None, 0, dict(C_of_fold, mean_score))"""
    from sklearn.model_selection import GridSearchCV
    from sklearn.svm import SVC

    folds = int(fold.max()) + 1
    pred = np.full(len(labels), -1, dtype=np.int32)
    C_of_fold, mean_score = np.zeros(folds), np.zeros((folds, len(Cs)))
    for f in range(folds):
        train, test = fold != f, fold == f
        clf = GridSearchCV(SVC(), {"C": list(Cs)}, cv=cv, scoring="accuracy", verbose=0).fit(emb[train], labels[train])
        pred[test] = clf.predict(emb[test])
        C_of_fold[f], mean_score[f] = clf.best_params_["C"], clf.cv_results_["mean_test_score"]
    return pred, None, 0, dict(C_of_fold=C_of_fold, mean_score=mean_score)


def search_device(emb, labels, fold, Cs, cv, device, engine=None):
    """-> (pred int32 [N], decision float64 [N, pairs], total SMO iterations of the search and the refit, dict(C_of_fold,
    mean_score))"""
    import torch

    from .. import _cabi
    from ..svc import SVCEngine, inner_fold_table

    engine = engine if engine is not None else SVCEngine()
    x = torch.from_numpy(np.ascontiguousarray(emb, dtype=np.float32)).to(torch.device(device))
    folds = int(fold.max()) + 1
    res = engine.search_fit_predict_folds(x, labels, fold, inner_fold_table(labels, fold, cv, folds), Cs, folds=folds, inner=cv)
    engine.check_status(res, allow_iter_cap=True)
    if (int(res["status"].cpu()[0]) | int(res["search_status"].cpu()[0])) & _cabi.STATUS_SVC_ITER_CAP:
        print("warning: a problem stopped at the iteration cap before tol was reached")
    if int(res["search_status"].cpu()[0]) & _cabi.STATUS_SVC_MISSING_CLASS:
        print("warning: an inner training side lacks a class that its held-out side has; those rows count as wrong")
    iterations = int(res["iters"].sum()) + int(res["search_iters"].sum())
    return (res["pred"].cpu().numpy(), res["decision"].cpu().numpy(), iterations,
            dict(C_of_fold=res["C_of_fold"], mean_score=res["mean_score"]))


def evaluate(emb, labels, seed=0, C=1e5, device="cpu", engine=None, folds=FOLDS, search=False, search_C=SEARCH_C, search_cv=5):
    """-> (result {"Micro-F1": mean accuracy over the folds, "folds": n, "iterations": SMO iterations or 0}, detail dict(pred,
    fold, decision or None); pred holds the corpus' own label values, -1 for a row without a vote).  ``engine``: a gcc_amd.svc.SVCEngine (injectable for the emulator tests); sklearn when ``device``
    is "cpu" and no engine is given.  ``search``: the grid search over ``search_C`` with ``search_cv`` inner folds instead of
    ``C``; result then also holds "C", the winners per fold, and detail C_of_fold and mean_score."""
    labels = np.asarray(labels)
    if emb.shape[0] != len(labels):
        raise ValueError(f"{emb.shape[0]} embedding rows for {len(labels)} labelled graphs")
    classes, y = np.unique(labels, return_inverse=True)           # sorted, as sklearn orders them
    if len(classes) < 2:
        raise ValueError("graph classification needs at least two classes")
    fold = fold_ids(y, seed, folds)
    found = {}
    if search:
        Cs = [float(c) for c in search_C]
        if engine is None and str(device) == "cpu":
            pred, decision, iterations, found = search_sklearn(emb, y, fold, Cs, search_cv)
        else:
            pred, decision, iterations, found = search_device(emb, y, fold, Cs, search_cv, device, engine)
    elif engine is None and str(device) == "cpu":
        pred, decision, iterations = classify_sklearn(emb, y, fold, C)
    else:
        pred, decision, iterations = classify_device(emb, y, fold, C, device, engine)
    accuracies = [float((pred[fold == f] == y[fold == f]).mean()) for f in range(folds)]
    result = {"Micro-F1": float(np.mean(accuracies)), "folds": folds, "iterations": iterations}
    if search:
        result["C"] = [float(c) for c in found["C_of_fold"]]
    # a row without a vote (its fold trained none of the pairs) counts as wrong above and is stored as -1
    return result, dict(pred=np.where(pred >= 0, classes[np.maximum(pred, 0)], -1), fold=fold, decision=decision, **found)


def load_labels(a):
    from .. import ingest

    if a.tudataset and getattr(a, "tu_parse", "host") == "device":   # (all three files: the errors are those of --load-path)
        from ..tu_ingest import TUIngestEngine

        return TUIngestEngine(device=a.device).read_tudataset(a.tudataset, a.dataset)["graph_labels"]
    if a.tudataset:
        return ingest.read_tudataset(a.tudataset, a.dataset)["graph_labels"]
    z = np.load(a.graphs_npz)
    if "graph_labels" not in z:
        raise ValueError(f"{a.graphs_npz} holds no graph_labels")
    return z["graph_labels"].astype(np.int64)


def embed_corpus(a, pipeline=None):
    """the corpus embedded with the checkpoint ``--load-path`` (gcc_amd.generate.run) -> float32 [graphs, hidden]"""
    return checkpoint_table(a.load_path, a.dataset, a.device, a.batch_size, pipeline, tu_parse=a.tu_parse, graphs_npz=a.graphs_npz, tudataset=a.tudataset)


def main(argv=None, pipeline=None, engine=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", required=True, help="the corpus' name, e.g. imdb-binary")
    ap.add_argument("--emb-path", default=None)
    ap.add_argument("--load-path", default=None, help="checkpoint: embed the corpus on the device instead of reading --emb-path")
    ap.add_argument("--batch-size", type=int, default=256, help="--load-path: graphs embedded per batch")
    ap.add_argument("--tudataset", default=None, metavar="DIR")
    ap.add_argument("--graphs-npz", default=None)
    ap.add_argument("--tu-parse", choices=["host", "device"], default="host", help="--tudataset: parse the three files on the host (np.loadtxt) or on the device (gcc_text_ints_sep, gcc_tu_corpus)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--C", type=float, default=None, help="the box bound (default 100000); not with --search")
    ap.add_argument("--search", action="store_true", help="the reference's search=True: a grid search over C per fold, then a refit")
    ap.add_argument("--search-C", default=",".join("%g" % c for c in SEARCH_C), metavar="C1,C2,...", help="--search: the candidates")
    ap.add_argument("--search-cv", type=int, default=5, help="--search: inner folds")
    ap.add_argument("--save-pred", default=None, metavar="OUT.npz")
    ap.add_argument("--model", default="from_numpy_graph", help="the reference's option: only from_numpy_graph exists")
    ap.add_argument("--hidden-size", type=int, default=None, help="the reference's option: checked against the table's width")
    ap.add_argument("--num-shuffle", type=int, default=10, help="the reference's option: unused there as here")
    a = ap.parse_args(argv)
    if a.model != "from_numpy_graph":
        ap.error("--model: the reference's task asserts from_numpy_graph")
    if (a.emb_path is None) == (a.load_path is None):
        ap.error("pass --emb-path, or --load-path to embed the corpus")
    if (a.tudataset is None) == (a.graphs_npz is None):
        ap.error("pass --tudataset DIR or --graphs-npz F (the labels come from the corpus; dataset files are not bundled)")
    if a.tu_parse == "device" and a.tudataset is None:
        ap.error("--tu-parse device says where the files of --tudataset are parsed: pass --tudataset")
    if a.tu_parse == "device" and str(a.device) == "cpu":
        ap.error("--tu-parse device needs a GPU --device: the TU reader has no CPU path")
    if a.search and a.C is not None:
        ap.error("--C and --search exclude each other: the search picks C from --search-C")
    try:
        search_C = [float(c) for c in a.search_C.split(",")]
    except ValueError:
        ap.error(f"--search-C {a.search_C!r}: expected a comma-separated list of numbers")
    if a.search and (not search_C or min(search_C) <= 0 or a.search_cv < 2):
        ap.error("--search-C needs positive candidates and --search-cv at least 2")
    labels = load_labels(a)
    emb = embed_corpus(a, pipeline) if a.load_path is not None else load_embedding(a.emb_path)
    if a.hidden_size is not None and emb.shape[1] != a.hidden_size:
        ap.error(f"--hidden-size {a.hidden_size}, but the table has {emb.shape[1]} columns")
    result, detail = evaluate(emb, labels, a.seed, 100000.0 if a.C is None else a.C, a.device, engine, search=a.search,
                              search_C=search_C, search_cv=a.search_cv)
    if a.save_pred is not None:
        extra = {} if detail["decision"] is None else dict(decision=detail["decision"])
        if a.search:
            extra.update(C_of_fold=detail["C_of_fold"], mean_score=detail["mean_score"])
        np.savez(a.save_pred, pred=detail["pred"], fold=detail["fold"], labels=labels, **extra)
    print(result)
    return result


if __name__ == "__main__":
    main()
