"""Generates tests/golden/svc_fixtures.npz and svc_fixtures.json: the inputs of the C-SVC tests (tests/svc_check.py) and what
sklearn's SVC -- the reference's own classifier, gcc/tasks/graph_classification.py:61 -- measures on them.

Binary fixtures (a)-(e): unit-norm float32 rows, two classes, 90 % of the rows train (fold id 1), the rest are held out
(fold id 0).  Stored per fixture in the JSON: sklearn's support-vector counts with tol = 1e-3 (its default) and tol = 1e-7
(the converged answer), the max-abs gap of the default fit's held-out decision values to the converged fit's (the yardstick of
the device's tolerance: 4 x that gap, floored at 1e-4), and the smallest converged |decision|.  "device" holds the gap of
the device's decision values to the converged fit as measured when the fixtures were made (emulator / MI355X); the tests
measure it again and assert.

Multi-class fixtures m3 / m5: 3 and 5 classes, the last class with fewer than 10 rows, three stratified folds.
"tie": a 3-class set and one held-out row whose three pairwise decisions form a cycle (found by a seeded search with sklearn,
margins above 0.05), so every class gets one vote and libsvm answers the lowest class.
Run from the repo root:  python tests/golden/make_svc_fixtures.py
"""
import json
import os

import numpy as np
from sklearn.model_selection import StratifiedKFold
from sklearn.svm import SVC

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (rows, columns, shift, seed, conflicting duplicates, C)
BINARY = dict(a=(200, 16, 0.3, 1, 0, 1e5), b=(400, 64, 0.15, 2, 0, 1e5), c=(200, 64, 0.15, 3, 5, 1e5),
              d=(300, 2, 0.3, 4, 0, 100.0), e=(300, 4, 0.5, 5, 10, 1e5))


def unit(X):
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def binary(n, D, shift, seed, dup):
    rng = np.random.RandomState(seed)
    y = (np.arange(n) % 2).astype(np.int32)
    X = rng.randn(n, D) + shift * (2 * y[:, None] - 1)
    fold = np.ones(n, np.int32)
    fold[rng.permutation(n)[: n // 10]] = 0
    tr = np.nonzero(fold == 1)[0]
    X = unit(X)
    for k in range(dup):                                          # a training row again, bit for bit, with the opposite label
        X[tr[2 * k + 1]] = X[tr[2 * k]]
        y[tr[2 * k + 1]] = 1 - y[tr[2 * k]]
    return X, y, fold


def multiclass(classes, seed, n=150, D=8, small=7):
    rng = np.random.RandomState(seed)
    y = np.concatenate([np.arange(n - small) % (classes - 1), np.full(small, classes - 1)]).astype(np.int32)
    centres = 0.8 * rng.randn(classes, D)
    X = unit(centres[y] + rng.randn(n, D))
    fold = np.zeros(n, np.int32)
    for f, (_, te) in enumerate(StratifiedKFold(3, shuffle=True, random_state=seed).split(X, y)):
        fold[te] = f
    return X, y, fold


def vote_tie():
    for seed in range(100000):
        rng = np.random.RandomState(seed)
        y = np.repeat(np.arange(3), 3).astype(np.int32)
        X = unit(rng.randn(9, 2) + 0.5)
        q = unit(rng.randn(1, 2) + 0.5)
        dec = SVC(C=1e5, decision_function_shape="ovo").fit(X, y).decision_function(q)[0]     # (0,1), (0,2), (1,2): > 0 votes the lower
        cyc = (dec[0] > 0) == (dec[2] > 0) and (dec[0] > 0) != (dec[1] > 0)
        if cyc and np.abs(dec).min() > 0.05:
            return np.concatenate([X, q]), np.concatenate([y, [2]]).astype(np.int32), np.array([1] * 9 + [0], np.int32), dec
    raise RuntimeError("no vote cycle found")


def main():
    arrays, meta = {}, {}
    for name, (n, D, shift, seed, dup, C) in BINARY.items():
        X, y, fold = binary(n, D, shift, seed, dup)
        tr, te = fold == 1, fold == 0
        sk, conv = SVC(C=C).fit(X[tr], y[tr]), SVC(C=C, tol=1e-7).fit(X[tr], y[tr])
        d0, d1 = sk.decision_function(X[te]), conv.decision_function(X[te])
        meta[name] = dict(C=C, rows=n, columns=D, train=int(tr.sum()), sv_default=int(sk.n_support_.sum()),
                          sv_converged=int(conv.n_support_.sum()), gap_default_to_converged=float(np.abs(d0 - d1).max()),
                          min_abs_decision=float(np.abs(d1).min()), device={})
        arrays.update({f"{name}_x": X, f"{name}_y": y, f"{name}_fold": fold})
    for name, classes, seed in (("m3", 3, 11), ("m5", 5, 12)):
        X, y, fold = multiclass(classes, seed)
        arrays.update({f"{name}_x": X, f"{name}_y": y, f"{name}_fold": fold})
        meta[name] = dict(C=1e5, classes=classes, rows=len(y), smallest_class=int(np.bincount(y).min()))
    X, y, fold, dec = vote_tie()
    arrays.update(tie_x=X, tie_y=y, tie_fold=fold)
    meta["tie"] = dict(C=1e5, sklearn_decision=dec.tolist())
    old = os.path.join(HERE, "svc_fixtures.json")
    if os.path.exists(old):                                       # keep the device's recorded figures
        for name, m in json.load(open(old)).items():
            if name in meta and "device" in m:
                meta[name]["device"] = m["device"]
    np.savez_compressed(os.path.join(HERE, "svc_fixtures.npz"), **arrays)
    json.dump(meta, open(old, "w"), indent=1)
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
