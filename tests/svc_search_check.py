"""The grid search over C on the device (gcc_svc_search_*, gcc_amd/csrc/svc.hip; SVCEngine.search_fit_predict_folds), shared by the
emulator tier (tests/test_svc_search_emu.py) and the GPU tier (tests/test_svc_search_gpu.py): the same cases and checks; only the
library, the pointer function and the device differ.

Two yardsticks.  The composition of the existing engine: a search is, per outer fold o and candidate c, what ``fit_predict_folds``
computes on the outer fold's training rows as a corpus of their own with the inner folds as its folds -- same rows, same order, same
gamma, same distances (an entry of the distance matrix is one chain over the columns wherever it stands), cold start -- so the
counts, the iteration numbers and alpha are compared bit for bit, without a tolerance; so is the refit against the plain call at
the fold's winner.  And sklearn's GridSearchCV at the reference's shape (10 x 5 x 6) on tests/golden/graphcls_search_reference.npz,
a corpus on which no decision value is within the solvers' tolerance of zero (make_graphcls_search_golden.py), so winners, counts
and accuracy are reproduced exactly."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import gcc_amd.svc as svc_module
from gcc_amd import _cabi
from gcc_amd.svc import SVCEngine, inner_fold_table
from gcc_amd.tasks._common import fold_ids
from tests.svc_check import GOLDEN, UNBOUNDED, Svc  # noqa: F401  (Svc: the tiers build it)

SEARCH_KEYS_INT = ("correct", "search_iters", "search_problem_rows", "search_first_rows", "search_rows", "search_status", "best_index")
SEARCH_KEYS_F64 = ("search_alpha", "search_rho", "mean_score", "C_of_fold", "inner_gamma")
REFIT_KEYS_INT = ("pred", "iters", "n_free", "n_bounded", "problem_rows", "first_rows", "rows", "status")
REFIT_KEYS_F64 = ("decision", "rho", "obj", "alpha", "gamma")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def search(S, X, y, outer, inner_tab, Cs, **kw):
    res = S.engine.search_fit_predict_folds(S.t(X), y, outer, inner_tab, Cs, **kw)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def stratified(y, folds, seed):
    with warnings.catch_warnings():                                # (a class smaller than the fold count: sklearn warns and splits)
        warnings.simplefilter("ignore")
        return fold_ids(y, seed, folds)


def inner_table(y, outer, inner):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return inner_fold_table(y, outer, inner)


# ------------------------------------------------------------------------------------------------------------- fixtures
def small():
    """N = 150 (no multiple of 64), D = 16, three classes, one of 4 rows; outer 3, inner 3"""
    rng = np.random.RandomState(11)
    y = np.concatenate([np.arange(146) % 2, np.full(4, 2)]).astype(np.int32)[rng.permutation(150)]
    X = 0.45 * rng.randn(3, 16)[y] + rng.randn(150, 16)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    outer = stratified(y, 3, 0)
    return dict(X=X, y=y, outer=outer, inner=inner_table(y, outer, 3), Cs=(0.5, 50.0, 5000.0), n_outer=3, n_inner=3)


def wide():
    """N = 2,400, two classes, outer 2, inner 2: inner problems of 600 rows (above the one-wave limit of 512), refits of 1,200"""
    rng = np.random.RandomState(12)
    y = (np.arange(2400) % 2).astype(np.int32)
    X = rng.randn(2400, 8) + 0.6 * (2 * y[:, None] - 1)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    outer = stratified(y, 2, 0)
    return dict(X=X, y=y, outer=outer, inner=inner_table(y, outer, 2), Cs=(1.0, 10.0), n_outer=2, n_inner=2)


FIXTURES = dict(small=small, wide=wide)
_cache = {}


def fixture(name):
    if ("fx", name) not in _cache:
        _cache["fx", name] = FIXTURES[name]()
    return _cache["fx", name]


def searched(S, name, Cs=None, per_launch=UNBOUNDED):
    """one search per (tier, fixture, candidates, launch split), shared by the tests and left unchanged"""
    fx = fixture(name)
    Cs = fx["Cs"] if Cs is None else Cs
    key = (id(S), name, tuple(Cs), per_launch)
    if key not in _cache:
        _cache[key] = search(S, fx["X"], fx["y"], fx["outer"], fx["inner"], Cs, iters_per_launch=per_launch)
    return _cache[key]


# -------------------------------------------------------------------------------------- 1. the composition, bit for bit
def check_equals_composition(S, name):
    fx = fixture(name)
    X, y, outer, inner, Cs = fx["X"], fx["y"], fx["outer"], fx["inner"], fx["Cs"]
    res = searched(S, name)
    classes, n_inner = int(y.max()) + 1, fx["n_inner"]
    assert res["status"][0] == 0 and res["search_status"][0] == 0
    assert res["correct"].shape == (fx["n_outer"], len(Cs), n_inner) and res["correct"].dtype == np.int32
    total = 0
    for o in range(fx["n_outer"]):
        tr = np.nonzero(outer != o)[0]
        ids = inner[o, tr]
        assert np.array_equal(res["inner_sizes"][o], np.bincount(ids, minlength=n_inner))
        for c, C in enumerate(Cs):
            one = S.fit(X[tr], y[tr], ids, C=C, classes=classes, folds=n_inner, iters_per_launch=UNBOUNDED)
            assert one["status"][0] == 0
            counts = [int((one["pred"][ids == i] == y[tr][ids == i]).sum()) for i in range(n_inner)]
            assert res["correct"][o, :, :][c].tolist() == counts, (o, C)
            assert np.array_equal(res["search_iters"][o, :, :, c], one["iters"]), (o, C)
            assert np.array_equal(bits(res["search_rho"][o, :, :, c]), bits(one["rho"])), (o, C)
            assert np.array_equal(bits(res["inner_gamma"][o]), bits(one["gamma"]))
            assert np.array_equal(res["search_problem_rows"][o], one["problem_rows"])
            assert np.array_equal(res["search_first_rows"][o], one["first_rows"])
            for i in range(n_inner):
                for pair in range(one["pairs"]):
                    n = int(one["problem_rows"][i, pair])
                    assert np.array_equal(res["search_rows"][o, i, pair, :n], tr[one["rows"][i, pair, :n]])
                    assert np.array_equal(bits(res["search_alpha"][o, i, pair, c, :n]), bits(one["alpha"][i, pair, :n])), (o, C, i, pair)
            total += int(one["iters"].sum())
    assert int(res["search_iters"].sum()) == total
    # the refit: the plain call at the fold's winner, on that fold
    assert np.array_equal(res["C_of_fold"], np.asarray(Cs)[res["best_index"]])
    for C in sorted(set(res["C_of_fold"].tolist())):
        plain = S.fit(X, y, outer, C=C, classes=classes, folds=fx["n_outer"], iters_per_launch=UNBOUNDED)
        for o in np.nonzero(res["C_of_fold"] == C)[0]:
            te = outer == o
            assert np.array_equal(res["pred"][te], plain["pred"][te]) and np.array_equal(bits(res["decision"][te]), bits(plain["decision"][te]))
            for key in ("iters", "n_free", "n_bounded", "problem_rows", "first_rows", "rows"):
                assert np.array_equal(res[key][o], plain[key][o]), (key, o)
            for key in ("rho", "obj", "alpha", "gamma"):
                assert np.array_equal(bits(res[key][o]), bits(plain[key][o])), (key, o)
    print(f"{name}: {int(res['search_iters'].sum())} search + {int(res['iters'].sum())} refit iterations, winners {res['C_of_fold'].tolist()}")
    return res


def check_four_wave(S):
    res = check_equals_composition(S, "wide")
    assert res["search_problem_rows"].min() == 600 and res["problem_rows"].min() == 1200


# -------------------------------------------------------------------------------------------------------- 2. launch split
def check_launch_split(S, name="small", per_launch=37):
    whole, split = searched(S, name), searched(S, name, per_launch=per_launch)
    assert whole["search_launches"] == 1 and whole["launches"] == 1
    assert split["search_launches"] >= max(2, int(whole["search_iters"].max()) // per_launch)
    assert split["launches"] >= max(2, int(whole["iters"].max()) // per_launch)
    for key in SEARCH_KEYS_INT + REFIT_KEYS_INT:
        assert np.array_equal(whole[key], split[key]), key
    for key in SEARCH_KEYS_F64 + REFIT_KEYS_F64:
        assert np.array_equal(bits(whole[key]), bits(split[key])), key


# ------------------------------------------------------------------------------------------------------ 3. ties and order
def check_ties_and_mean(S):
    """candidates (10, 10, 1): the two 10s score the same, so wherever 10 wins the winner is entry 0; the mean score is
    np.mean of the fold accuracies, bit for bit"""
    res = searched(S, "small", Cs=(10.0, 10.0, 1.0))
    assert np.array_equal(res["correct"][:, 0], res["correct"][:, 1])
    assert np.array_equal(res["search_iters"][..., 0], res["search_iters"][..., 1])
    assert not (res["best_index"] == 1).any()
    for o in range(3):
        acc = [[res["correct"][o, c, i] / res["inner_sizes"][o, i] for i in range(3)] for c in range(3)]
        mean = np.array([np.mean(a) for a in acc])
        assert np.array_equal(bits(res["mean_score"][o]), bits(mean))
        assert res["best_index"][o] == int(np.argmax(mean)) and res["C_of_fold"][o] == (10.0, 10.0, 1.0)[res["best_index"][o]]
        ten_wins = mean[0] >= mean[2]
        assert res["best_index"][o] == (0 if ten_wins else 2)


# ------------------------------------------------------------------------------------- 4. sklearn, the reference's shape
def golden():
    if "golden" not in _cache:
        z = np.load(os.path.join(GOLDEN, "graphcls_search_reference.npz"))
        meta = json.load(open(os.path.join(GOLDEN, "graphcls_search_reference.json")))
        _, y = np.unique(z["graph_labels"], return_inverse=True)
        outer = fold_ids(y, meta["seed"], 10)
        _cache["golden"] = dict(X=z["emb"], y=y.astype(np.int32), outer=outer, inner=inner_fold_table(y, outer, meta["cv"]), meta=meta)
    return _cache["golden"]


def sklearn_counts():
    """sklearn's own count table on the golden corpus: GridSearchCV's split scores times the fold sizes"""
    if "sk_counts" not in _cache:
        from sklearn.model_selection import GridSearchCV
        from sklearn.svm import SVC

        g = golden()
        Cs, cv = g["meta"]["Cs"], g["meta"]["cv"]
        counts = np.zeros((10, len(Cs), cv), dtype=np.int64)
        for o in range(10):
            tr = g["outer"] != o
            grid = GridSearchCV(SVC(), {"C": Cs}, cv=cv, scoring="accuracy").fit(g["X"][tr], g["y"][tr])
            sizes = np.bincount(g["inner"][o, tr], minlength=cv)
            for i in range(cv):
                counts[o, :, i] = np.rint(grid.cv_results_[f"split{i}_test_score"] * sizes[i])
        _cache["sk_counts"] = counts
    return _cache["sk_counts"]


def check_against_sklearn(S):
    g = golden()
    meta = g["meta"]
    res = search(S, g["X"], g["y"], g["outer"], g["inner"], meta["Cs"])
    assert res["status"][0] == 0 and res["search_status"][0] == 0
    print(f"golden: {int(res['search_iters'].sum())} search + {int(res['iters'].sum())} refit iterations (sklearn's n_iter_ total "
          f"{meta['total_n_iter']}), winners {res['C_of_fold'].tolist()}")
    assert res["C_of_fold"].tolist() == [float(c) for c in meta["winners"]]
    assert len(set(meta["winners"])) >= 2
    assert np.array_equal(res["correct"], sklearn_counts())
    assert np.array_equal(bits(res["mean_score"]), bits(np.array(meta["mean_score"])))
    y, outer = g["y"], g["outer"]
    accuracy = np.mean([float((res["pred"][outer == f] == y[outer == f]).mean()) for f in range(10)])
    assert accuracy == meta["result"]["Micro-F1"]


# ---------------------------------------------------------------------------------------------------------------- 5. edges
def edge_corpus(n=60):
    rng = np.random.RandomState(5)
    y = (np.arange(n) % 2).astype(np.int32)
    X = rng.randn(n, 6) + 0.8 * (2 * y[:, None] - 1)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    outer = ((np.arange(n) // 2) % 2).astype(np.int32)             # both classes in both folds
    inner = np.full((2, n), -1, dtype=np.int32)
    for o in range(2):
        tr = np.nonzero(outer != o)[0]
        inner[o, tr] = (np.arange(len(tr)) // 2) % 2
    return X, y, outer, inner


def check_inner_missing_class(S):
    """class 2 has one row on each outer training side: the inner problems that hold it out never learn the class -- the bit is the
    inner problems' own, the refit has the class, and the run succeeds"""
    X, y, outer, inner = edge_corpus()
    y = y.copy()
    y[0], y[2] = 2, 2                                             # rows 0 (outer fold 0) and 2 (outer fold 1)
    res = search(S, X, y, outer, inner, (1.0, 100.0), classes=3, folds=2, inner=2)
    assert res["search_status"][0] == _cabi.STATUS_SVC_MISSING_CLASS and res["status"][0] == 0
    S.engine.check_status({k: torch.from_numpy(res[k]) for k in ("status", "search_status")})
    # the held-out row of class 2 counts as wrong; the composition says the same
    for o in range(2):
        tr = np.nonzero(outer != o)[0]
        for c, C in enumerate((1.0, 100.0)):
            one = S.fit(X[tr], y[tr], inner[o, tr], C=C, classes=3, folds=2)
            assert one["status"][0] == _cabi.STATUS_SVC_MISSING_CLASS
            counts = [int((one["pred"][inner[o, tr] == i] == y[tr][inner[o, tr] == i]).sum()) for i in range(2)]
            assert res["correct"][o, c].tolist() == counts
    assert (res["pred"] >= 0).all()


def check_single_class_inner_side(S, monkeypatch):
    X, y, outer, inner = edge_corpus()
    y = y.copy()
    tr = np.nonzero(outer != 0)[0]
    y[tr[inner[0, tr] != 1]] = 0                                  # outer fold 0, inner fold 1: the training side is class 0 alone
    calls = []
    monkeypatch.setattr(S.engine, "invoke", lambda *a, **k: calls.append(a))
    with pytest.raises(ValueError, match="outer fold 0, inner fold 1"):
        S.engine.search_fit_predict_folds(S.t(X), y, outer, inner, (1.0, 10.0))
    assert not calls


def check_limits(S):
    X, y, outer, inner = edge_corpus()
    with pytest.raises(RuntimeError, match=r"candidates 17 outside 1\.\.GCC_SVC_SEARCH_MAX_CANDIDATES \(16\)"):
        S.engine.search_fit_predict_folds(S.t(X), y, outer, inner, np.arange(1.0, 18.0))
    with pytest.raises(RuntimeError, match=r"inner 17 outside 2\.\.GCC_SVC_SEARCH_MAX_INNER \(16\)"):
        S.engine.search_fit_predict_folds(S.t(X), y, outer, inner, (1.0,), inner=17)
    with pytest.raises(RuntimeError, match=r"inner 1 outside 2\.\.GCC_SVC_SEARCH_MAX_INNER \(16\)"):
        S.engine.search_fit_predict_folds(S.t(X), y, outer, np.where(inner >= 0, 0, -1), (1.0,), inner=1)
    q = S.lib.gcc_svc_search_workspace_bytes
    assert q(100, 8, 3, 64, 16, 10, 50, 40) > 100 * 100 * 4       # 30,720 problems
    assert q(100, 8, 3, 64, 16, 11, 50, 40) < 0                   # 33,792
    err = S.lib.gcc_last_error().decode()
    assert "33792 inner problems" in err and "GCC_SVC_SEARCH_MAX_PROBLEMS (32768)" in err
    for args, text in (((100, 8, 2, 65, 3, 2, 50, 40), "folds 65"), ((100, 8, 2, 3, 3, 2, 4097, 40), "max_rows 4097"),
                       ((100, 8, 2, 3, 3, 2, 50, 51), "max_inner_rows 51"), ((100, 8, 2, 3, 3, 0, 50, 40), "candidates 0")):
        assert q(*args) < 0 and text in S.lib.gcc_last_error().decode(), args
    # the entry points themselves refuse, and launch nothing: a NULL member by name
    a = _cabi.GccSvcSearchArgs()
    a.N, a.D, a.classes, a.folds, a.inner, a.candidates, a.max_rows, a.max_inner_rows = 60, 6, 2, 2, 2, 2, 30, 15
    a.iters_per_launch, a.eps = 10, 1e-3
    ws, status = torch.zeros(1 << 20, dtype=torch.uint8, device=S.device), torch.zeros(1, dtype=torch.int32, device=S.device)
    for name in ("setup", "solve", "score", "refit", "predict"):
        with pytest.raises(RuntimeError, match=f"gcc_svc_search_{name}: search_status is NULL"):
            S.engine.invoke(f"gcc_svc_search_{name}", a, ws, status)


def check_status_bits(S):
    X, y, outer, inner = edge_corpus()
    kw = dict(classes=2, folds=2, inner=2, iter_cap=200)
    assert search(S, X, y, outer, inner, (1.0, 10.0), **kw)["status"][0] == 0
    bad = y.copy()
    bad[7], bad[8] = 2, -1
    res = search(S, X, bad, outer, inner, (1.0, 10.0), **kw)
    assert res["status"][0] == _cabi.STATUS_SVC_BAD_LABEL and res["search_status"][0] & _cabi.STATUS_SVC_BAD_LABEL
    assert res["problem_rows"][0, 0] == int((outer != 0).sum()) - int((outer[[7, 8]] != 0).sum())
    badf = outer.copy()
    badf[9], badf[10] = 2, -1
    res = search(S, X, y, badf, inner, (1.0, 10.0), **kw)
    assert res["status"][0] == _cabi.STATUS_SVC_BAD_FOLD and res["pred"][9] == -1 and res["pred"][10] == -1
    assert (np.delete(res["pred"], [9, 10]) >= 0).all()
    nan = X.copy()
    nan[17, 3], nan[40, 0] = np.nan, np.inf
    res = search(S, nan, y, outer, inner, (1.0, 10.0), **kw)
    assert res["status"][0] & _cabi.STATUS_SVC_NONFINITE
    with pytest.raises(RuntimeError, match="NaN or infinite"):
        S.engine.check_status(dict(status=torch.from_numpy(res["status"])))
    with pytest.raises(ValueError, match=r"inner_of_row\[0\] must hold an inner fold"):
        S.engine.search_fit_predict_folds(S.t(X), y, outer, np.where(inner == 1, 5, inner), (1.0,), inner=2)


def check_iteration_cap_only_warns(S):
    X, y, outer, inner = edge_corpus()
    res = search(S, X, y, outer, inner, (1e5,), iter_cap=3)
    assert res["search_status"][0] == _cabi.STATUS_SVC_ITER_CAP and res["status"][0] == _cabi.STATUS_SVC_ITER_CAP
    assert (res["search_iters"] == 3).all() and (res["iters"] == 3).all()
    result = {k: torch.from_numpy(res[k]) for k in ("status", "search_status")}
    with pytest.raises(RuntimeError, match="iteration cap"):
        S.engine.check_status(result)
    S.engine.check_status(result, allow_iter_cap=True)


def check_short_workspace(S, monkeypatch):
    """a workspace sized for smaller problems than the labels make: every problem is refused on the device, nothing is counted, and
    nothing is written past the workspace that was asked for"""
    X, y, outer, inner = edge_corpus()
    monkeypatch.setattr(svc_module, "largest_problem", lambda *a: 10)
    engine = SVCEngine(S.lib, S.ptr)
    engine._workspace = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device=S.device)
    res = engine.search_fit_predict_folds(S.t(X), y, outer, inner, (1.0, 10.0))
    nbytes = res["workspace_bytes"]
    assert nbytes < (1 << 20) and bool((engine._workspace[nbytes:] == 0xA5).all())
    assert int(res["status"].cpu()[0]) == _cabi.STATUS_SVC_OVERFLOW and int(res["search_status"].cpu()[0]) == _cabi.STATUS_SVC_OVERFLOW
    assert (res["correct"] == 0).all() and (res["pred"].cpu().numpy() == -1).all()
    assert (res["search_iters"].cpu().numpy() == 0).all() and (res["search_problem_rows"].cpu().numpy() > 10).all()
    with pytest.raises(RuntimeError, match="more rows than"):
        engine.check_status(res)
