"""Node classification on frozen embeddings (gcc/tasks/node_classification.py of the reference, the "GCC (freeze)" column of the
paper's node-classification table): ``StratifiedKFold(10, shuffle=True, random_state=seed)`` over ``label_matrix.argmax(1)``,
a one-vs-rest ``LogisticRegression(C=1000)`` per fold, per held-out row the k classes of highest probability (k = the row's label
count; a row without labels gets every class, the reference's ``argsort()[-0:]``), micro-F1 per fold, the mean as
``{"Micro-F1": ...}``.

    python -m gcc_amd.tasks.node_classification --dataset usa_airport --emb-path E.npy (--edgelist F --nodelabel F | --labels-npz F) \\
        [--seed 0] [--device cuda:0|cpu] [--C 1000] [--solver lbfgs|liblinear] [--save-pred OUT.npz]
    python -m gcc_amd.tasks.node_classification --dataset usa_airport --load-path CKPT --edgelist F --nodelabel F ...
    python -m gcc_amd.tasks.node_classification --dataset usa_airport --model prone --hidden-size 64 --edgelist F --nodelabel F \\
        [--prone-seed S] [--save-emb OUT.npy]
    python -m gcc_amd.tasks.node_classification --dataset usa_airport --model graphwave --hidden-size 64 --edgelist F --nodelabel F \\
        [--save-emb OUT.npy]

The feature matrix is the table itself, row i for node i.  The labels come from gcc_amd.ingest.read_edgelist (h-index datasets:
above / not above the median) or from key ``y`` [N, classes] of ``--labels-npz``.  With ``--load-path`` the nodes are embedded on
the device with the checkpoint first (what ``generate.py --edgelist`` does).  On a GPU all folds and classes are fitted in one
pass of gcc_amd.logreg.LogRegEngine (gcc_amd/csrc/logreg.hip), which computes the minimiser of sklearn's objective; ``--device
cpu`` runs sklearn itself, fold by fold, as the reference does.  ``--solver lbfgs`` is the intercept-unpenalised objective of
scikit-learn >= 0.22, ``liblinear`` the one of the reference's pinned 0.20.3 (the intercept penalised as a feature).
``--model from_numpy --hidden-size --num-shuffle`` of the reference's command line are accepted and checked, nothing more.
``--model prone`` is the reference's ProNE baseline (gcc/models/emb/prone.py): the table is computed from ``--edgelist`` first, on
the device by gcc_amd.prone.ProNEEngine (gcc_amd/csrc/prone.hip) or, with ``--device cpu``, by its float64 NumPy restatement;
``--hidden-size`` (default 64) is its width, ``--prone-seed`` (default ``--seed``) the seed of the range finder's test matrix.
``--model graphwave`` is the reference's GraphWave baseline (gcc/models/emb/graphwave.py): the table of characteristic-function
samples of the heat wavelets, on the device by gcc_amd.graphwave.GraphWaveEngine (gcc_amd/csrc/graphwave.hip) or, with ``--device
cpu``, by its float64 NumPy restatement; ``--hidden-size`` (default 64, a multiple of 4) is its width.  It draws nothing.
Prints the reference's result line with the fold count and the Newton iterations added; ``--save-pred`` stores the predicted
label sets, the folds, the decision values and the labels."""
from __future__ import annotations

import argparse

import numpy as np

from ._common import FOLDS, baseline_table, checkpoint_table, fold_ids, load_embedding
SOLVERS = {"lbfgs": 0.0, "liblinear": 1.0}      # -> the intercept's penalty


def top_k(decision, k):
    """the reference's TopKRanker.predict on decision values: per row the k[r] highest (decision descending, then class
    ascending); k = 0 selects every class -> uint8 [rows, classes]"""
    n, classes = decision.shape
    pred = np.zeros((n, classes), dtype=np.uint8)
    for r in range(n):
        order = sorted(range(classes), key=lambda c: (-decision[r, c], c))
        pred[r, order[: int(k[r]) if k[r] > 0 else classes]] = 1
    return pred


def fold_f1(tp, fp, fn):
    """micro-F1 as sklearn computes it: 2 tp / (2 tp + fp + fn), 0 without any positive"""
    den = 2 * tp + fp + fn
    return float(2 * tp / den) if den > 0 else 0.0


def classify_sklearn(emb, y, fold, C, solver):
    """node_classification.py:64-79 with the folds given: sklearn's one-vs-rest LogisticRegression per fold and the reference's
    own ranking (argsort of the probabilities) -> (pred uint8 [N, classes], None, counts [folds, 3], 0)"""
    from sklearn.linear_model import LogisticRegression
    from sklearn.multiclass import OneVsRestClassifier

    folds = int(fold.max()) + 1
    emb = np.asarray(emb, dtype=np.float64)                        # (the reference's features_matrix is float64)
    pred = np.zeros(y.shape, dtype=np.uint8)
    counts = np.zeros((folds, 3), dtype=np.int64)
    for f in range(folds):
        train, test = fold != f, fold == f
        clf = OneVsRestClassifier(LogisticRegression(C=C, solver=solver)).fit(emb[train], y[train])
        probs = np.asarray(clf.predict_proba(emb[test]))
        rows = np.nonzero(test)[0]
        for i, r in enumerate(rows):
            k = int(y[r].sum())
            pred[r, clf.classes_[probs[i].argsort()[-k:]]] = 1     # (k = 0: the whole row, as the reference)
        counts[f] = _counts(pred[test], y[test])
    return pred, None, counts, 0


def _counts(pred, y):
    p, t = pred != 0, y != 0
    return int((p & t).sum()), int((p & ~t).sum()), int((~p & t).sum())


def classify_device(emb, y, fold, C, solver, device, engine=None):
    """-> (pred uint8 [N, classes], decision float64 [N, classes], counts [folds, 3], total Newton iterations)"""
    import torch

    from .. import _cabi
    from ..logreg import LogRegEngine

    engine = engine if engine is not None else LogRegEngine()
    x = torch.from_numpy(np.ascontiguousarray(emb, dtype=np.float32)).to(torch.device(device))
    res = engine.fit_predict_folds(x, y, fold, C=C, intercept_penalty=SOLVERS[solver])
    engine.check_status(res, allow_iter_cap=True)
    if int(res["status"].cpu()[0]) & _cabi.STATUS_LR_ITER_CAP:
        print("warning: a (fold, class) problem stopped at the iteration cap before tol was reached")
    return (res["pred"].cpu().numpy(), res["decision"].cpu().numpy(), res["counts"].cpu().numpy().astype(np.int64),
            int(res["iters"].sum()))


def evaluate(emb, y, seed=0, C=1000.0, solver="lbfgs", device="cpu", engine=None, folds=FOLDS):
    """-> (result {"Micro-F1": mean over the folds, "folds": n, "iterations": Newton iterations or 0}, detail dict(pred, fold,
    decision or None)).  ``engine``: a gcc_amd.logreg.LogRegEngine (injectable for the emulator tests); sklearn when ``device``
    is "cpu" and no engine is given."""
    y = (np.asarray(y) != 0).astype(np.float32)
    if y.ndim != 2 or emb.shape[0] != y.shape[0]:
        raise ValueError(f"{emb.shape[0]} embedding rows for a label matrix of shape {y.shape}")
    if solver not in SOLVERS:
        raise ValueError(f"solver {solver!r}: one of {sorted(SOLVERS)}")
    fold = fold_ids(y.argmax(axis=1), seed, folds)
    if engine is None and str(device) == "cpu":
        pred, decision, counts, iterations = classify_sklearn(emb, y, fold, C, solver)
    else:
        pred, decision, counts, iterations = classify_device(emb, y, fold, C, solver, device, engine)
    scores = [fold_f1(*(int(v) for v in counts[f])) for f in range(folds)]
    result = {"Micro-F1": sum(scores) / len(scores), "folds": folds, "iterations": iterations}
    return result, dict(pred=pred, fold=fold, decision=decision)


def load_labels(a):
    from .. import ingest

    if a.labels_npz is not None:
        z = np.load(a.labels_npz)
        if "y" not in z:
            raise ValueError(f"{a.labels_npz} holds no y")
        return z["y"]
    return ingest.read_edgelist(a.edgelist, a.nodelabel, hindex="hindex" in a.dataset)["y"]


def embed_nodes(a, pipeline=None):
    """the nodes embedded with the checkpoint ``--load-path`` (gcc_amd.generate.run) -> float32 [nodes, hidden]"""
    return checkpoint_table(a.load_path, a.dataset, a.device, a.batch_size, pipeline, edgelist=a.edgelist, nodelabel=a.nodelabel)


def embed_prone(a, prone_engine=None):
    """the ProNE table of ``--edgelist`` (gcc/tasks/__init__.py: build_model("prone")) -> float32 [nodes, hidden]"""
    from .. import ingest

    g = ingest.read_edgelist(a.edgelist)
    return baseline_table("prone", g["row_ptr"], g["col_idx"], 64 if a.hidden_size is None else a.hidden_size, a.device, prone_engine,
                          seed=a.seed if a.prone_seed is None else a.prone_seed)


def embed_graphwave(a, graphwave_engine=None):
    """the GraphWave table of ``--edgelist`` (gcc/tasks/__init__.py: build_model("graphwave")) -> float32 [nodes, hidden]"""
    from .. import ingest
    from ..graphwave import check_width

    g = ingest.read_edgelist(a.edgelist)
    d = 64 if a.hidden_size is None else a.hidden_size
    check_width(d)
    return baseline_table("graphwave", g["row_ptr"], g["col_idx"], d, a.device, graphwave_engine)


def main(argv=None, pipeline=None, engine=None, prone_engine=None, graphwave_engine=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", required=True, help="the corpus' name, e.g. usa_airport (a name with 'hindex': median labels)")
    ap.add_argument("--emb-path", default=None)
    ap.add_argument("--load-path", default=None, help="checkpoint: embed the nodes on the device instead of reading --emb-path")
    ap.add_argument("--batch-size", type=int, default=256, help="--load-path: nodes embedded per batch")
    ap.add_argument("--edgelist", default=None)
    ap.add_argument("--nodelabel", default=None)
    ap.add_argument("--labels-npz", default=None, help="key y [N, classes]: the label matrix of a corpus without dataset files")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--C", type=float, default=1000.0)
    ap.add_argument("--solver", default="lbfgs", choices=sorted(SOLVERS),
                    help="lbfgs: the intercept unpenalised (scikit-learn >= 0.22); liblinear: penalised (the reference's 0.20.3)")
    ap.add_argument("--save-pred", default=None, metavar="OUT.npz")
    ap.add_argument("--model", default="from_numpy", help="the reference's option: from_numpy (a frozen table), prone or graphwave (the baselines)")
    ap.add_argument("--hidden-size", type=int, default=None,
                    help="the reference's option: checked against the table's width; --model prone / graphwave: the width (default 64)")
    ap.add_argument("--prone-seed", type=int, default=None, help="--model prone: the seed of the range finder's test matrix (default --seed)")
    ap.add_argument("--save-emb", default=None, metavar="OUT.npy", help="--model prone / graphwave: store the float32 table")
    ap.add_argument("--num-shuffle", type=int, default=10, help="the reference's option: unused there as here")
    a = ap.parse_args(argv)
    if a.model not in ("from_numpy", "prone", "graphwave"):
        ap.error("--model: only from_numpy (a frozen embedding table), prone and graphwave (the baselines) are served")
    if a.model in ("prone", "graphwave"):
        if a.emb_path is not None or a.load_path is not None:
            ap.error(f"--model {a.model} computes the table: it takes neither --emb-path nor --load-path")
        if a.edgelist is None or a.nodelabel is None or a.labels_npz is not None:
            ap.error(f"--model {a.model} needs --edgelist F --nodelabel F")
        if a.model == "graphwave" and a.prone_seed is not None:
            ap.error("--prone-seed goes with --model prone (GraphWave draws nothing)")
        if a.model == "graphwave" and a.hidden_size is not None and (a.hidden_size % 4 != 0 or not 4 <= a.hidden_size <= 256):
            ap.error(f"--model graphwave: --hidden-size {a.hidden_size} must be a multiple of 4 in 4..256")
    elif a.save_emb is not None or a.prone_seed is not None:
        ap.error("--save-emb goes with --model prone / graphwave, --prone-seed with --model prone")
    elif (a.emb_path is None) == (a.load_path is None):
        ap.error("pass --emb-path, or --load-path to embed the nodes")
    files = a.edgelist is not None or a.nodelabel is not None
    if files == (a.labels_npz is not None) or (files and (a.edgelist is None or a.nodelabel is None)):
        ap.error("pass --edgelist F --nodelabel F, or --labels-npz F (dataset files are not bundled)")
    if a.load_path is not None and a.edgelist is None:
        ap.error("--load-path embeds the nodes of --edgelist")
    y = load_labels(a)
    if a.model in ("prone", "graphwave"):
        emb = embed_prone(a, prone_engine) if a.model == "prone" else embed_graphwave(a, graphwave_engine)
        if a.save_emb is not None:
            np.save(a.save_emb, emb)
    else:
        emb = embed_nodes(a, pipeline) if a.load_path is not None else load_embedding(a.emb_path)
    if a.hidden_size is not None and emb.shape[1] != a.hidden_size:
        ap.error(f"--hidden-size {a.hidden_size}, but the table has {emb.shape[1]} columns")
    result, detail = evaluate(emb, y, a.seed, a.C, a.solver, a.device, engine)
    if a.save_pred is not None:
        extra = {} if detail["decision"] is None else dict(decision=detail["decision"])
        np.savez(a.save_pred, pred=detail["pred"], fold=detail["fold"], labels=np.asarray(y), **extra)
    print(result)
    return result


if __name__ == "__main__":
    main()
