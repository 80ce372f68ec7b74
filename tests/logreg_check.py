"""The logistic-regression kernels (gcc_amd/csrc/logreg.hip) against sklearn's converged fits and a float64 NumPy Newton
iteration (tests/logreg_reference.py), shared by the emulator tier (tests/test_logreg_emu.py) and the GPU tier
(tests/test_logreg_gpu.py): the same cases and checks; only the library, the pointer function and the device differ.

The device computes the minimiser of sklearn's objective, not sklearn's default iterate.  Tolerance per fixture: two converged
sklearn fits (newton-cholesky and lbfgs, tol = 1e-12) and the NumPy Newton are made here on the same float32 rows, and
``tol_fix = 4 x max(|lbfgs - nc|, |numpy - nc|)`` over the held-out decision values; the device's held-out decision values, coef
and intercept must lie within tol_fix of newton-cholesky's.  With intercept_penalty = 1 the yardsticks are liblinear
(tol = 1e-12) and the NumPy Newton.  Both yardsticks are references, never the code under test;
tests/golden/logreg_fixtures.json records the figures of the day the fixtures were chosen.

The fixtures are generated, not stored: unit-norm rows around two centres, a random tenth held out as fold 0 (fold 1 holds the
rest, so its problem trains on the tenth; only fold 0 is compared)."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch
from sklearn.linear_model import LogisticRegression
from sklearn.model_selection import StratifiedKFold
from sklearn.multiclass import OneVsRestClassifier

from gcc_amd import _cabi
from gcc_amd.logreg import LogRegEngine
from tests import logreg_reference as R

C = 1000.0
TOL = 1e-9
# name -> rows, columns, distance of the centres, seed
FIXTURES = {"sep": (150, 4, 3.0, 11), "a": (300, 8, 0.5, 12), "d1": (200, 1, 1.0, 13), "t15": (240, 15, 0.5, 14),
            "t16": (240, 16, 0.5, 15), "t17": (240, 17, 0.5, 16), "onepos": (300, 16, 0.5, 17), "stride": (300, 8, 0.5, 18),
            "nltd": (60, 64, 0.2, 19), "w64": (600, 64, 0.15, 20), "c256": (400, 256, 0.2, 21), "c129": (300, 129, 0.2, 22),
            "c128": (300, 128, 0.2, 23)}
EMU_FIXTURES = ["sep", "a", "d1", "t15", "t16", "t17", "onepos", "stride"]      # N <= 300, D <= 17
GPU_FIXTURES = EMU_FIXTURES + ["nltd", "w64", "c128", "c129", "c256"]           # wider shapes; D = 128 is the last Cholesky in LDS
PENALISED = ["a", "t16"]                                                        # also with intercept_penalty = 1


class Lr:
    """the library under test, its pointer function and its device (the emulator works on CPU tensors)"""

    def __init__(self, lib, ptr, device):
        self.lib, self.ptr, self.device = lib, ptr, torch.device(device)
        self.engine = LogRegEngine(lib, ptr)

    def t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def fit(self, X, y, fold, extra=0, **kw):
        """``extra``: columns of 1e30 behind every row, which must not be read (a row stride larger than D)"""
        x = self.t(X)
        if extra:
            wide = torch.full((X.shape[0], X.shape[1] + extra), 1e30, dtype=torch.float32, device=self.device)
            wide[:, : X.shape[1]] = x
            x = wide[:, : X.shape[1]]
        res = self.engine.fit_predict_folds(x, y, fold, **kw)
        return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def rows(n, D, classes, sep, seed):
    rng = np.random.RandomState(seed)
    cls = np.arange(n) % classes
    X = rng.randn(n, D) + sep * rng.randn(classes, D)[cls]
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32), cls, rng


@functools.lru_cache(maxsize=None)
def fixture(name):
    n, D, sep, seed = FIXTURES[name]
    X, cls, rng = rows(n, D, 2, sep, seed)
    fold = np.ones(n, dtype=np.int32)
    fold[rng.permutation(n)[: n // 10]] = 0
    t = (cls == 0).astype(np.uint8)
    if name == "onepos":                         # a single positive training row (of fold 0's problem)
        t[:] = 0
        t[np.nonzero(fold == 1)[0][7]] = 1
    return dict(X=X, t=t, y=t[:, None], fold=fold, extra=5 if name == "stride" else 0)


@functools.lru_cache(maxsize=None)
def yardstick(name, rho=0.0):
    """the references on a binary fixture, fitted once and shared: held-out decision values, coef and intercept of fold 0"""
    fx = fixture(name)
    X, t, tr, te = fx["X"], fx["t"], fx["fold"] == 1, fx["fold"] == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if rho == 0.0:
            main = LogisticRegression(C=C, solver="newton-cholesky", tol=1e-12, max_iter=1000).fit(X[tr], t[tr])
            other = LogisticRegression(C=C, tol=1e-12, max_iter=100000).fit(X[tr], t[tr])
        else:
            main = LogisticRegression(C=C, solver="liblinear", tol=1e-12, max_iter=100000).fit(X[tr], t[tr])
            other = None
    w, b, iters, gmax = R.newton(X[tr], t[tr], C, rho, TOL)
    dec_main, dec_np = main.decision_function(X[te]), X[te].astype(np.float64) @ w + b
    gap_np = float(np.abs(dec_np - dec_main).max())
    gap_sk = float(np.abs(other.decision_function(X[te]) - dec_main).max()) if other is not None else 0.0
    return dict(dec=dec_main, coef=main.coef_[0].astype(np.float64), intercept=float(main.intercept_[0]), gap_np=gap_np, gap_sk=gap_sk,
                tol=4.0 * max(gap_np, gap_sk), np_iters=iters)


# ----------------------------------------------------------------------------------------------------------- binary fits
def check_fit(S, name, rho=0.0):
    """checks 1 and 2: the fit against the references, and optimality recomputed in NumPy from the returned coef / intercept"""
    fx, ref = fixture(name), yardstick(name, rho)
    X, t, fold = fx["X"], fx["t"], fx["fold"]
    tr, te = fold == 1, fold == 0
    res = S.fit(X, fx["y"], fold, extra=fx["extra"], intercept_penalty=rho)
    assert res["status"][0] == 0 and res["state"][0, 0] == _cabi.LR_CONVERGED
    coef, b = res["coef"][0, 0], float(res["intercept"][0, 0])
    gap_dec = float(np.abs(res["decision"][te, 0] - ref["dec"]).max())
    gap_coef, gap_b = float(np.abs(coef - ref["coef"]).max()), abs(b - ref["intercept"])
    print(f"{name} rho {rho:g}: iterations {res['iters'][0, 0]} (NumPy {ref['np_iters']}) in {res['syncs']} syncs; references apart "
          f"{ref['gap_sk']:.3e} (sklearn pair) / {ref['gap_np']:.3e} (NumPy), allowed {ref['tol']:.3e}; device: decision {gap_dec:.3e}, "
          f"coef {gap_coef:.3e}, intercept {gap_b:.3e}")
    assert gap_dec <= ref["tol"] and gap_coef <= ref["tol"] and gap_b <= ref["tol"]
    assert np.abs(res["decision"][te, 0] - (X[te].astype(np.float64) @ coef + b)).max() <= 1e-12       # decision = w . x + b
    # the stop rule plus the rounding of at most 65,536 terms <= 1, which is below 1e-11
    gn = R.grad_norm(X[tr], t[tr], coef, b, C, rho)
    print(f"{name} rho {rho:g}: max|g| / C recomputed {gn:.3e}, reported {res['grad'][0, 0]:.3e}")
    assert res["grad"][0, 0] <= TOL and gn <= 2 * TOL
    return res


# ------------------------------------------------------------------------------------------------------------- sync split
OUTPUTS = ("pred", "decision", "counts", "coef", "intercept", "iters", "grad", "state", "status")


def check_sync_split(S, fit):
    """``fit(iters_per_sync=...)`` -> result: 1, 3 and 200 iterations per host read give bit-equal outputs"""
    runs = {ips: fit(iters_per_sync=ips) for ips in (1, 3, 200)}
    most = int(runs[200]["iters"].max())
    assert most >= 4
    for ips, res in runs.items():
        assert res["syncs"] == max(1, math.ceil(most / ips)), (ips, res["syncs"], most)
        for key in OUTPUTS:
            assert res[key].tobytes() == runs[200][key].tobytes(), (ips, key)
    return runs[200]


# --------------------------------------------------------------------------------------- top-k, ties and constant columns
@functools.lru_cache(maxsize=None)
def rule_fixture():
    """120 x 6 rows around three centres, seven label columns, three folds.  Columns 0 and 1 are identical (class 0's rows);
    2 and 6 are the other two classes; 3 and 5 are all ones except on the unlabelled row; 4 occurs in fold 0 only.  Rows 0 and 3
    (fold 0) sit at class 0's centre but carry the labels {2, 3, 5}: k = 3 picks the two +inf columns and one of the tied
    columns 0 / 1.  Row 6 (fold 0) has no label, row 9 (fold 0) has all seven."""
    X, cls, _ = rows(120, 6, 3, 2.0, 31)
    y = np.zeros((120, 7), dtype=np.uint8)
    y[cls == 0, 0] = y[cls == 0, 1] = 1
    y[cls == 1, 2] = 1
    y[cls == 2, 6] = 1
    y[:, 3] = y[:, 5] = 1
    fold = ((np.arange(120) // 3) % 3).astype(np.int32)
    for r in (0, 3, 6, 9):
        fold[r] = 0
    y[[0, 3]] = [0, 0, 1, 1, 0, 1, 0]
    y[6] = 0
    y[9] = 1
    y[np.nonzero(fold == 0)[0][10:14], 4] = 1
    return X, y, fold


def check_rules(S):
    X, y, fold = rule_fixture()
    res = S.fit(X, y, fold)
    assert res["status"][0] == 0
    dec, pred, state = res["decision"], res["pred"], res["state"]
    # identical columns: the same problem twice, bit for bit, and the lower class wins where k cuts between them
    assert dec[:, 0].tobytes() == dec[:, 1].tobytes() and np.isfinite(dec[:, 0]).all()
    assert pred[0].tolist() == [1, 0, 0, 1, 0, 1, 0] and pred[3].tolist() == [1, 0, 0, 1, 0, 1, 0]
    assert not ((pred[:, 1] == 1) & (pred[:, 0] == 0)).any()
    # a row without labels is given every class; so is the row that has them all
    assert pred[6].tolist() == [1] * 7 and pred[9].tolist() == [1] * 7
    # constant columns: all ones on fold 0's training side -> +inf there, solved where the unlabelled row trains
    assert state[0, 3] == state[0, 5] == _cabi.LR_ALL_ONE and (dec[fold == 0][:, [3, 5]] == np.inf).all()
    assert state[1, 3] == state[2, 5] == _cabi.LR_CONVERGED and np.isfinite(dec[fold != 0][:, [3, 5]]).all()
    # absent from fold 0's training side -> -inf there, solved elsewhere
    assert state[0, 4] == _cabi.LR_ALL_ZERO and (dec[fold == 0, 4] == -np.inf).all() and res["iters"][0, 4] == 0
    assert state[1, 4] == state[2, 4] == _cabi.LR_CONVERGED and np.isfinite(dec[fold != 0, 4]).all() and res["iters"][1, 4] > 0
    assert res["intercept"][0, 4] == -np.inf and res["intercept"][0, 3] == np.inf and (res["coef"][0, 3] == 0).all()
    # the whole rule, restated in NumPy on the device's own decision values
    assert np.array_equal(pred, R.top_k(dec, y))
    assert np.array_equal(res["counts"], R.counts(pred, y, fold, 3))
    return res


# ---------------------------------------------------------------------------------------- multi-label, ten folds, sklearn
MULTI_SEED = 1


@functools.lru_cache(maxsize=None)
def multi_fixture(seed=MULTI_SEED):
    """240 x 16, four classes, 15 % of the rows with a second label, the reference's ten folds"""
    X, cls, rng = rows(240, 16, 4, 0.6, seed)
    y = np.eye(4, dtype=np.uint8)[cls]
    second = rng.rand(240) < 0.15
    y[np.nonzero(second)[0], (cls[second] + 1) % 4] = 1
    fold = np.zeros(240, dtype=np.int32)
    for f, (_, te) in enumerate(StratifiedKFold(10, shuffle=True, random_state=0).split(X, y.argmax(1))):
        fold[te] = f
    return X, y, fold


@functools.lru_cache(maxsize=None)
def multi_yardstick(seed=MULTI_SEED):
    """converged sklearn one-vs-rest per fold -> (decision [N, 4] of every row's own fold, tol_fix over all of them)"""
    X, y, fold = multi_fixture(seed)
    dec = np.zeros(y.shape)
    gap = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for f in range(10):
            tr, te = fold != f, fold == f
            nc = OneVsRestClassifier(LogisticRegression(C=C, solver="newton-cholesky", tol=1e-12, max_iter=1000)).fit(X[tr], y[tr])
            lb = OneVsRestClassifier(LogisticRegression(C=C, tol=1e-12, max_iter=100000)).fit(X[tr], y[tr])
            dec[te] = nc.decision_function(X[te])
            gap = max(gap, float(np.abs(lb.decision_function(X[te]) - dec[te]).max()))
            for c in range(4):
                w, b, _, _ = R.newton(X[tr], y[tr, c], C, 0.0, TOL)
                gap = max(gap, float(np.abs(X[te].astype(np.float64) @ w + b - dec[te, c]).max()))
    return dec, 4.0 * gap


def cut_gaps(dec, y):
    """per row the distance between its k-th and (k + 1)-th decision value (inf where k is 0 or every class)"""
    ordered = -np.sort(-dec, axis=1)
    k = (y != 0).sum(1)
    out = np.full(len(dec), np.inf)
    inner = (k > 0) & (k < dec.shape[1])
    out[inner] = ordered[inner, k[inner] - 1] - ordered[inner, k[inner]]
    return out


def check_multilabel(S):
    X, y, fold = multi_fixture()
    dec, tol = multi_yardstick()
    sure = cut_gaps(dec, y) > 2 * tol
    print(f"multi-label: tol_fix {tol:.3e}, smallest cut gap {cut_gaps(dec, y).min():.3e}, rows left out {(~sure).sum()}")
    assert (~sure).sum() <= 0.02 * len(y)                # (holds for the converged sklearn fit alone: the seed was picked for it)
    res = S.fit(X, y, fold)
    assert res["status"][0] == 0 and (res["state"] == _cabi.LR_CONVERGED).all()
    assert float(np.abs(res["decision"] - dec).max()) <= tol
    assert np.array_equal(res["pred"][sure], R.top_k(dec, y)[sure])
    assert np.array_equal(res["counts"], R.counts(res["pred"], y, fold, 10))
    return res


# --------------------------------------------------------------------------------------------------- status and refusals
def check_status_bits(S):
    fx = fixture("a")
    X, y, fold = fx["X"], fx["y"], fx["fold"]

    def sentence(res, text, **kw):
        with pytest.raises(RuntimeError, match=text):
            S.engine.check_status(dict(status=torch.from_numpy(res["status"])), **kw)

    for bad in (np.nan, np.inf):
        Xb = X.copy()
        Xb[17, 3] = bad
        res = S.fit(Xb, y, fold)
        assert res["status"][0] == _cabi.STATUS_LR_NONFINITE and (res["state"] == _cabi.LR_NOT_RUN).all() and (res["iters"] == 0).all()
        sentence(res, "NaN or infinite")
    badf = fold.copy()
    badf[9], badf[10] = 2, -1
    res = S.fit(X, y, badf, folds=2)
    assert res["status"][0] == _cabi.STATUS_LR_BAD_FOLD and (res["pred"][[9, 10]] == 0).all() and (res["decision"][[9, 10]] == 0).all()
    assert res["state"][0, 0] == _cabi.LR_CONVERGED
    sentence(res, "fold id outside")
    res = S.fit(X, y, fold, iter_cap=1)
    assert res["status"][0] == _cabi.STATUS_LR_ITER_CAP and res["iters"][0, 0] == 1 and res["state"][0, 0] == _cabi.LR_CAPPED
    assert res["syncs"] == 1
    sentence(res, "iteration cap")
    S.engine.check_status(dict(status=torch.from_numpy(res["status"])), allow_iter_cap=True)
    for bit, text in ((_cabi.STATUS_LR_PIVOT, "non-positive pivot"), (_cabi.STATUS_LR_LINE_SEARCH, "no decrease")):
        sentence(dict(status=np.array([bit], dtype=np.int32)), text)


def check_refusals(S):
    q = S.lib.gcc_logreg_workspace_bytes
    assert q(65536, 256, 1, 1) > 3 * 65536 * 8
    for args, text in (((65537, 8, 2, 10), "N 65537 outside 1..GCC_LR_MAX_ROWS"), ((0, 8, 2, 10), "N 0"),
                       ((100, 257, 2, 10), "D 257 outside 1..GCC_LR_MAX_DIM"), ((100, 0, 2, 10), "D 0"),
                       ((100, 8, 257, 10), "classes 257 outside 1..GCC_LR_MAX_CLASSES"), ((100, 8, 0, 10), "classes 0"),
                       ((100, 8, 2, 17), "folds 17 outside 1..GCC_LR_MAX_FOLDS"), ((100, 8, 2, 0), "folds 0")):
        assert q(*args) < 0 and S.lib.gcc_last_error().decode().startswith("gcc_logreg_workspace_bytes: " + text), args
    with pytest.raises(RuntimeError, match="classes 257"):
        S.engine.fit_predict_folds(S.t(np.zeros((300, 2), np.float32)), np.zeros((300, 257), np.uint8), np.arange(300) % 10)
    with pytest.raises(RuntimeError, match="folds 17"):
        S.engine.fit_predict_folds(S.t(np.zeros((300, 2), np.float32)), np.zeros((300, 2), np.uint8), np.arange(300) % 17)
    # a short workspace and NULL members, through the C calls themselves
    import ctypes

    X, y, fold = S.t(np.zeros((64, 4), np.float32)), S.t(np.zeros((64, 2), np.uint8)), S.t(np.zeros(64, np.int32))
    out = {k: S.t(np.zeros(shape, dt)) for k, shape, dt in (("pred", (64, 2), np.uint8), ("status", 1, np.int32), ("unfinished", 1, np.int32))}
    need = q(64, 4, 2, 1)
    ws = S.t(np.zeros(need, np.uint8))

    def args(**kw):
        a = _cabi.GccLogregArgs()
        a.emb, a.ld, a.N, a.D, a.classes, a.folds = X.data_ptr(), 4, 64, 4, 2, 1
        a.y, a.fold_of_row, a.pred, a.unfinished = y.data_ptr(), fold.data_ptr(), out["pred"].data_ptr(), out["unfinished"].data_ptr()
        a.iters_per_sync, a.iter_cap, a.C, a.tol, a.intercept_penalty = 4, 200, C, TOL, 0.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    stream = _cabi.raw_stream(S.device)

    def refused(name, a, nbytes, status, text):
        rc = getattr(S.lib, name)(ctypes.byref(a), ws.data_ptr(), nbytes, status, stream)
        assert rc < 0 and text in S.lib.gcc_last_error().decode(), (name, S.lib.gcc_last_error().decode())

    st = out["status"].data_ptr()
    for name in ("gcc_logreg_setup", "gcc_logreg_step", "gcc_logreg_predict"):
        refused(name, args(), need - 1, st, f"{name}: workspace_bytes {need - 1} is less than gcc_logreg_workspace_bytes ({need})")
        refused(name, args(y=None), need, st, f"{name}: y is NULL")
        refused(name, args(emb=None), need, st, f"{name}: emb is NULL")
        refused(name, args(fold_of_row=None), need, st, f"{name}: fold_of_row is NULL")
        refused(name, args(), need, None, f"{name}: status is NULL")
        refused(name, args(ld=3), need, st, "ld 3 must be at least D (4)")
        refused(name, args(N=65537), need, st, "N 65537")
    refused("gcc_logreg_step", args(unfinished=None), need, st, "gcc_logreg_step: unfinished is NULL")
    refused("gcc_logreg_predict", args(pred=None), need, st, "gcc_logreg_predict: pred is NULL")
    refused("gcc_logreg_setup", args(iter_cap=0), need, st, "iter_cap 0")
    assert int(out["status"].cpu()[0]) == 0


def check_cpu_tensor_refused(lib):
    """the product path (the device pointer function) takes no CPU tensor, whatever the library"""
    engine = LogRegEngine(lib, _cabi.dev_ptr)
    with pytest.raises(RuntimeError, match="device \\(HIP\\) tensors only"):
        engine.fit_predict_folds(torch.zeros(20, 4), np.zeros((20, 2), np.uint8), np.arange(20) % 2)
