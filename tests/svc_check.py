"""The C-SVC kernels (gcc_amd/csrc/svc.hip) against sklearn's SVC -- the reference's own classifier -- on the fixtures of
tests/golden/svc_fixtures.npz, shared by the emulator tier (tests/test_svc_emu.py) and the GPU tier (tests/test_svc_gpu.py): the
same cases and checks; only the library, the pointer function and the device differ.

Tolerance of the decision values and of rho, per fixture: sklearn's default fit (tol = 1e-3) sits some gap from its converged
fit (tol = 1e-7); the device's gap to the converged fit may be at most 4 x that gap, floored at 1e-4.  Both sklearn fits are
made here, on the same float32 rows; svc_fixtures.json records the figures of the day the fixtures were made.

Sign: the device's decision values are libsvm's (positive votes for the lower class of the pair); sklearn negates them for
two classes, so binary comparisons negate sklearn's."""
import functools
import json
import os

import numpy as np
import pytest
import torch
from sklearn.svm import SVC

import gcc_amd.svc as svc_module
from gcc_amd import _cabi
from gcc_amd.svc import SVCEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-3
UNBOUNDED = 2 ** 31 - 1
DISTANCE_SHAPES = [(1, 1, 0), (63, 3, 0), (64, 64, 0), (65, 65, 0), (130, 256, 0), (130, 3, 5), (65, 256, 9), (64, 1, 2)]   # N, D, extra stride


class Svc:
    """the library under test, its pointer function and its device (the emulator works on CPU tensors)"""

    def __init__(self, lib, ptr, device):
        self.lib, self.ptr, self.device = lib, ptr, torch.device(device)
        self.engine = SVCEngine(lib, ptr)

    def t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def fit(self, X, y, fold, **kw):
        res = self.engine.fit_predict_folds(self.t(X), y, fold, **kw)
        return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}

    def d2(self, X):
        """the device's own distance matrix (tested against float64 by check_distances), float32 [N, N]"""
        return self.engine.distances(self.t(X))[0].cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def fixtures():
    z = np.load(os.path.join(GOLDEN, "svc_fixtures.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "svc_fixtures.json")))
    fx = {name: dict(X=z[name + "_x"], y=z[name + "_y"], fold=z[name + "_fold"], **m) for name, m in meta.items()}
    # generated, not stored: "w", 540 training rows (above 512 rows a problem runs in four waves with workgroup barriers), and
    # "x", 2,790 (above 2,730 rows the solver's LDS passes 64 KiB); unit-norm rows, two classes 0.15 apart, a tenth held out
    for name, n, D, seed in (("w", 600, 32, 21), ("x", 3100, 16, 22)):
        rng = np.random.RandomState(seed)
        y = (np.arange(n) % 2).astype(np.int32)
        X = rng.randn(n, D) + 0.15 * (2 * y[:, None] - 1)
        fx[name] = dict(X=(X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32), y=y,
                        fold=1 - np.isin(np.arange(n) % 20, (3, 14)).astype(np.int32), C=1e5)
    return fx


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """sklearn on a binary fixture, fitted once and shared: the default and the converged fit of fold 0"""
    fx = fixtures()[name]
    X, y, tr, te = fx["X"], fx["y"], fx["fold"] == 1, fx["fold"] == 0
    sk, conv = SVC(C=fx["C"]).fit(X[tr], y[tr]), SVC(C=fx["C"], tol=1e-7).fit(X[tr], y[tr])
    out = dict(dec_default=-sk.decision_function(X[te]), dec_conv=-conv.decision_function(X[te]), pred_conv=conv.predict(X[te]),
               rho_default=-float(sk._intercept_[0]), rho_conv=-float(conv._intercept_[0]),
               sv_default=int(sk.n_support_.sum()), sv_conv=int(conv.n_support_.sum()))
    alpha = np.zeros(int(tr.sum()))
    alpha[sk.support_] = np.abs(sk.dual_coef_[0])
    out["alpha_default"] = alpha                                  # in the order of X[tr]
    gap = float(np.abs(out["dec_default"] - out["dec_conv"]).max())
    out["gap"], out["tol"] = gap, max(4.0 * gap, 1e-4)
    return out


# ------------------------------------------------------------------------------------------------------------ distances
def check_distances(S, N, D, extra):
    rng = np.random.RandomState(N * 1000 + D)
    wide = np.full((N, D + extra), 1e30, dtype=np.float32)         # the columns past D must not be read
    wide[:, :D] = rng.randn(N, D).astype(np.float32)
    if N > 2:
        wide[2] = wide[0]                                         # a duplicate row: distance exactly 0
    d2, status = S.engine.distances(S.t(wide)[:, :D])
    d2 = d2.cpu().numpy()
    assert int(status.cpu()[0]) == 0
    assert np.array_equal(d2.view(np.int32), d2.T.view(np.int32)), "both triangles agree bit for bit"
    assert (np.diag(d2) == 0).all() and (d2 >= 0).all()
    if N > 2:
        assert d2[0, 2] == 0 and np.array_equal(d2[0], d2[2])
    x = wide[:, :D].astype(np.float64)
    ref = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    # every term (a - b)^2 carries two roundings, the chain of D additions one each: relative (D + 3) * 2^-24 at the most
    assert (np.abs(d2 - ref) <= (D + 3) * 2.0 ** -24 * ref).all()


def check_nonfinite(S):
    X = fixtures()["a"]["X"].copy()
    X[17, 3] = np.nan
    X[40, 0] = np.inf
    _, status = S.engine.distances(S.t(X))
    assert int(status.cpu()[0]) == _cabi.STATUS_SVC_NONFINITE
    fx = fixtures()["a"]
    res = S.fit(X, fx["y"], fx["fold"], iter_cap=200)
    assert res["status"][0] & _cabi.STATUS_SVC_NONFINITE
    with pytest.raises(RuntimeError, match="NaN or infinite"):
        S.engine.check_status(dict(status=torch.from_numpy(res["status"])))


# ---------------------------------------------------------------------------------------------------------- binary fits
def problem_arrays(S, fx, res, f=0, pair=0):
    """(rows, y, alpha, Q) of one solved problem: Q = y y^T K in float64 from the kernel values the solver itself uses,
    (float32) exp(-gamma d2) of the device's distances"""
    n, ni = int(res["problem_rows"][f, pair]), int(res["first_rows"][f, pair])
    rows = res["rows"][f, pair, :n].astype(np.int64)
    y = np.where(np.arange(n) < ni, 1.0, -1.0)
    d2 = S.d2(fx["X"])[np.ix_(rows, rows)].astype(np.float64)
    K = np.exp(-res["gamma"][f] * d2).astype(np.float32).astype(np.float64)
    return rows, y, res["alpha"][f, pair, :n], K * y[:, None] * y[None, :]


def kkt_gap(y, alpha, Q, C):
    G = Q @ alpha - 1.0
    up = np.where(y > 0, alpha < C, alpha > 0)
    low = np.where(y > 0, alpha > 0, alpha < C)
    return float((-y * G)[up].max() - (-y * G)[low].min())


def check_binary(S, name, **kw):
    fx, ref = fixtures()[name], yardstick(name)
    X, y, fold, C = fx["X"], fx["y"], fx["fold"], fx["C"]
    te = fold == 0
    res = S.fit(X, y, fold, C=C, **kw)
    assert res["status"][0] == 0
    n = int(res["problem_rows"][0, 0])
    assert n == int((~te).sum())
    # support vectors
    sv = int(res["n_free"][0, 0] + res["n_bounded"][0, 0])
    slack = max(1, int(0.01 * n)) if ref["sv_default"] != ref["sv_conv"] else 0
    print(f"{name}: iterations {res['iters'][0, 0]} in {res['launches']} launches, support vectors {sv} (sklearn {ref['sv_default']} / "
          f"{ref['sv_conv']}), bounded {res['n_bounded'][0, 0]}")
    assert abs(sv - ref["sv_default"]) <= slack
    # rho and decision values
    dec = res["decision"][te, 0]
    gap = float(np.abs(dec - ref["dec_conv"]).max())
    print(f"{name}: decision gap to the converged fit: sklearn default {ref['gap']:.3e}, device {gap:.3e}, allowed {ref['tol']:.3e}; "
          f"rho {res['rho'][0, 0]:.6f} (sklearn {ref['rho_default']:.6f} / {ref['rho_conv']:.6f})")
    assert gap <= ref["tol"]
    assert abs(res["rho"][0, 0] - ref["rho_conv"]) <= ref["tol"]
    # labels, wherever the converged decision is beyond the tolerance
    sure = np.abs(ref["dec_conv"]) > ref["tol"]
    assert (~sure).sum() <= 0.02 * te.sum()
    assert np.array_equal(res["pred"][te][sure], ref["pred_conv"][sure])
    assert np.array_equal(res["pred"][te], np.where(dec > 0, 0, 1))
    # KKT and the dual objective, recomputed in float64 from the returned alpha
    rows, yy, alpha, Q = problem_arrays(S, fx, res)
    assert np.array_equal(rows, np.concatenate([np.nonzero(~te & (y == 0))[0], np.nonzero(~te & (y == 1))[0]]))
    assert (alpha >= 0).all() and (alpha <= C).all() and abs(float(alpha @ yy)) <= 1e-9 * max(1.0, alpha.sum())
    assert int((alpha > 0).sum()) == sv and int((alpha >= C).sum()) == int(res["n_bounded"][0, 0])
    kkt = kkt_gap(yy, alpha, Q, C)
    obj = 0.5 * alpha @ Q @ alpha - alpha.sum()
    ytr = y[~te]
    a_sk = ref["alpha_default"][np.concatenate([np.nonzero(ytr == 0)[0], np.nonzero(ytr == 1)[0]])]     # in the problem's row order
    obj_sk = 0.5 * a_sk @ Q @ a_sk - a_sk.sum()
    print(f"{name}: KKT gap {kkt:.3e}; dual objective {obj:.9e} (reported {res['obj'][0, 0]:.9e}), sklearn default {obj_sk:.9e}")
    assert kkt < 2 * EPS
    assert abs(res["obj"][0, 0] - obj) <= 1e-9 * abs(obj) + 1e-9
    assert obj <= obj_sk + 1e-6 * abs(obj_sk)
    return res


def check_launch_split(S, name, per_launch=37):
    fx = fixtures()[name]
    whole = S.fit(fx["X"], fx["y"], fx["fold"], C=fx["C"], iters_per_launch=UNBOUNDED)
    split = S.fit(fx["X"], fx["y"], fx["fold"], C=fx["C"], iters_per_launch=per_launch)
    assert whole["launches"] == 1 and split["launches"] >= max(2, int(whole["iters"].max()) // per_launch)
    n = whole["problem_rows"]
    for key in ("pred", "iters", "n_free", "n_bounded", "problem_rows", "status"):
        assert np.array_equal(whole[key], split[key]), key
    for key in ("gamma", "decision", "rho", "obj"):
        assert np.array_equal(whole[key].view(np.int64), split[key].view(np.int64)), key
    for f in range(whole["folds"]):
        assert np.array_equal(whole["alpha"][f, 0, : n[f, 0]].view(np.int64), split["alpha"][f, 0, : n[f, 0]].view(np.int64))
    return whole


def check_iteration_cap(S):
    fx = fixtures()["d"]
    res = S.fit(fx["X"], fx["y"], fx["fold"], C=fx["C"], iters_per_launch=4096, iter_cap=100)
    assert res["status"][0] == _cabi.STATUS_SVC_ITER_CAP and res["iters"][0, 0] == 100 and res["launches"] == 1
    with pytest.raises(RuntimeError, match="iteration cap"):
        S.engine.check_status(dict(status=torch.from_numpy(res["status"])))
    S.engine.check_status(dict(status=torch.from_numpy(res["status"])), allow_iter_cap=True)


# ---------------------------------------------------------------------------------------------------------- multi-class
def check_multiclass(S, name):
    """every fold against SVC.predict, on every held-out row, and the one-vs-one decision values; the folds' small class has 4
    or 5 training rows"""
    fx = fixtures()[name]
    X, y, fold = fx["X"], fx["y"], fx["fold"]
    res = S.fit(X, y, fold, C=fx["C"])
    assert res["status"][0] == 0 and res["classes"] == fx["classes"] and res["pairs"] == fx["classes"] * (fx["classes"] - 1) // 2
    for f in range(3):
        tr, te = fold != f, fold == f
        conv = SVC(C=fx["C"], tol=1e-7, decision_function_shape="ovo").fit(X[tr], y[tr])
        sk = SVC(C=fx["C"], decision_function_shape="ovo").fit(X[tr], y[tr])
        d_conv = conv.decision_function(X[te])
        tol = max(4.0 * float(np.abs(sk.decision_function(X[te]) - d_conv).max()), 1e-4)
        gap = float(np.abs(res["decision"][te] - d_conv).max())
        print(f"{name} fold {f}: decision gap {gap:.3e}, allowed {tol:.3e}")
        assert gap <= tol
        assert np.array_equal(res["pred"][te], conv.predict(X[te]))          # every held-out row: vote order and ties as libsvm's
        assert np.array_equal(res["pred"][te], sk.predict(X[te]))
        sizes = np.bincount(y[tr], minlength=fx["classes"])
        pair = 0
        for ci in range(fx["classes"]):
            for cj in range(ci + 1, fx["classes"]):
                assert res["problem_rows"][f, pair] == sizes[ci] + sizes[cj] and res["first_rows"][f, pair] == sizes[ci]
                pair += 1


def check_vote_tie(S):
    """one vote each for the three classes: libsvm answers the lowest class"""
    fx = fixtures()["tie"]
    res = S.fit(fx["X"], fx["y"], fx["fold"], C=fx["C"])
    assert res["status"][0] == _cabi.STATUS_SVC_MISSING_CLASS       # fold 1 trains on the held-out row alone
    dec = res["decision"][9]
    assert np.allclose(dec, fx["sklearn_decision"], rtol=0, atol=1e-2) and (np.abs(dec) > 0.05).all()
    votes = np.bincount([0 if dec[0] > 0 else 1, 0 if dec[1] > 0 else 2, 1 if dec[2] > 0 else 2], minlength=3)
    assert votes.tolist() == [1, 1, 1] and res["pred"][9] == 0
    assert (res["pred"][:9] == -1).all() and (res["decision"][:9] == 0).all()       # fold 1 solved nothing: no vote


# ---------------------------------------------------------------------------------------------------------------- edges
def check_single_row_class_and_two_row_problem(S):
    rng = np.random.RandomState(3)
    X = rng.randn(12, 5)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    # fold 0 trains on rows 4..11: class 0 x 6, class 1 x 1, class 2 x 1 -> problems of 7, 7 and 2 rows
    y = np.array([0, 1, 2, 0, 0, 0, 0, 0, 0, 0, 1, 2], dtype=np.int32)
    fold = np.array([0, 0, 0, 0] + [1] * 8, dtype=np.int32)
    res = S.fit(X, y, fold, C=1e5, classes=3, folds=2)
    assert res["problem_rows"][0].tolist() == [7, 7, 2] and res["first_rows"][0].tolist() == [6, 6, 1]
    tr, te = fold == 1, fold == 0
    conv = SVC(C=1e5, tol=1e-7, decision_function_shape="ovo").fit(X[tr], y[tr])
    sk = SVC(C=1e5, decision_function_shape="ovo").fit(X[tr], y[tr])
    tol = max(4.0 * float(np.abs(sk.decision_function(X[te]) - conv.decision_function(X[te])).max()), 1e-4)
    assert np.abs(res["decision"][te] - conv.decision_function(X[te])).max() <= tol
    assert np.array_equal(res["pred"][te], conv.predict(X[te]))
    # the two-row problem: alpha_0 = alpha_1 = 1 / (1 - K_01), both free, rho = 0
    k01 = np.exp(-res["gamma"][0] * ((X[10].astype(np.float64) - X[11]) ** 2).sum())
    assert np.allclose(res["alpha"][0, 2, :2], 1.0 / (1.0 - k01), rtol=1e-5)
    assert res["n_free"][0, 2] == 2 and res["n_bounded"][0, 2] == 0 and abs(res["rho"][0, 2]) < 1e-9 and res["iters"][0, 2] == 1


def check_all_alpha_at_bound(S):
    fx = fixtures()["b"]
    X, y, fold = fx["X"][:100], fx["y"][:100], 1 - np.isin(np.arange(100) % 20, (0, 11)).astype(np.int32)
    res = S.fit(X, y, fold, C=0.01)
    n = int(res["problem_rows"][0, 0])
    assert n == 90 and res["n_bounded"][0, 0] == n and res["n_free"][0, 0] == 0 and res["status"][0] == 0
    assert (res["alpha"][0, 0, :n] == 0.01).all()
    tr, te = fold == 1, fold == 0
    conv = SVC(C=0.01, tol=1e-7).fit(X[tr], y[tr])
    assert np.abs(res["decision"][te, 0] + conv.decision_function(X[te])).max() <= 1e-4


def check_problem_size_limit(S):
    q = S.lib.gcc_svc_workspace_bytes
    assert q(8192, 64, 2, 10, 4096) > 8192 * 8192 * 4
    assert q(8192, 64, 2, 10, 4097) < 0
    err = S.lib.gcc_last_error().decode()
    assert err.startswith("gcc_svc_workspace_bytes: max_rows 4097") and "GCC_SVC_MAX_PROBLEM_ROWS (4096)" in err
    for args, text in (((16385, 64, 2, 10, 10), "N 16385"), ((100, 257, 2, 10, 10), "D 257"), ((100, 8, 1, 10, 10), "classes 1"),
                       ((100, 8, 33, 10, 10), "classes 33"), ((100, 8, 2, 0, 10), "folds 0"), ((100, 8, 2, 65, 10), "folds 65")):
        assert q(*args) < 0 and text in S.lib.gcc_last_error().decode(), args
    y = np.arange(9000) % 2
    with pytest.raises(RuntimeError, match="max_rows 8100 outside"):
        S.engine.fit_predict_folds(S.t(np.zeros((9000, 2), np.float32)), y, np.arange(9000) % 10)


def check_status_bits(S, monkeypatch):
    fx = fixtures()["a"]
    X, y, fold = fx["X"][:60], fx["y"][:60].copy(), np.ones(60, dtype=np.int32)
    fold[:6] = 0
    kw = dict(C=10.0, classes=2, folds=2)
    assert S.fit(X, y, fold, **kw)["status"][0] == 0
    bad = y.copy()
    bad[7], bad[8] = 2, -1
    res = S.fit(X, bad, fold, **kw)
    assert res["status"][0] == _cabi.STATUS_SVC_BAD_LABEL and res["problem_rows"][0, 0] == int((fold == 1).sum()) - 2
    assert (res["pred"] >= 0).all()
    badf = fold.copy()
    badf[9], badf[10] = 2, -1
    res = S.fit(X, y, badf, **kw)
    assert res["status"][0] == _cabi.STATUS_SVC_BAD_FOLD and res["pred"][9] == -1 and res["pred"][10] == -1
    assert (np.delete(res["pred"], [9, 10]) >= 0).all()
    lone = y.copy()
    lone[fold == 1] = 0                                           # class 1 only on fold 0's test side
    lone[0] = 1
    res = S.fit(X, lone, fold, **kw)
    assert res["status"][0] == _cabi.STATUS_SVC_MISSING_CLASS and (res["pred"][fold == 0] == -1).all()
    for bit, text in ((_cabi.STATUS_SVC_BAD_LABEL, "label outside"), (_cabi.STATUS_SVC_BAD_FOLD, "fold id outside"),
                      (_cabi.STATUS_SVC_MISSING_CLASS, "lacks a class"), (_cabi.STATUS_SVC_OVERFLOW, "more rows than")):
        with pytest.raises(RuntimeError, match=text):
            S.engine.check_status(dict(status=torch.tensor([bit], dtype=torch.int32)))
    # a workspace sized for smaller problems than the labels make: the problem is refused on the device, nothing is written past it
    monkeypatch.setattr(svc_module, "largest_problem", lambda *a: 20)
    res = S.fit(X, y, fold, **kw)
    assert res["status"][0] == _cabi.STATUS_SVC_OVERFLOW and (res["pred"][fold == 0] == -1).all()
    assert res["problem_rows"][0, 0] == int((fold == 1).sum()) and res["iters"][0, 0] == 0


def check_four_wave_kernel(S):
    """fixture "w": a problem of more than 512 rows is solved by four waves with workgroup barriers (fixtures (a)-(e) stay in
    one wave) -- the checks of the binary fixtures, and the launch split"""
    res = check_binary(S, "w")
    assert res["problem_rows"][0, 0] == 540
    check_launch_split(S, "w")


def check_large_lds_launch_split(S):
    """fixture "x": 2,790 rows per problem, 67 KiB of LDS -- the split into launches of 499 iterations equals one launch"""
    whole = check_launch_split(S, "x", per_launch=499)
    assert whole["problem_rows"][0, 0] == 2790 and whole["status"][0] == 0
