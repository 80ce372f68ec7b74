"""gcc_sim_search against a float64 NumPy restatement, shared by the emulator tier (tests/test_simsearch_emu.py) and the GPU
tier (tests/test_simsearch_gpu.py): the same cases, the same checks; only the library, the pointer function and the device
differ.

The order of a query's candidates is score descending, then column ascending.  The restatement states it with one lexsort.

Exact tier: integer entries in [-3, 3], normalize = 0.  Every product and partial sum is an integer below 9 * 256 < 2^24, so
the f32 scores are exact whatever the summation order and every output equals the restatement bit for bit; ties abound.

Normalised tier: Gaussian rows with planted matches.  The f32 score is the sum of D rounded products of unit-norm rows plus
the two normalisations: it differs from float64 by at most (D + 8) * 2^-24 <= 1.6e-5; the checks use DELTA = 4e-5 and hold
for every query without exception."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gcc_amd import _cabi
from gcc_amd.simsearch import SimilarityEngine

DELTA = 4e-5

# (mq, mc, D, k, splits, ld_extra, q_idx, c_idx, target): every (mq, mc) pair, D, k and splits of the list at least once;
# k > mc in "17x33"; mc never divisible by its splits; idx: None, "perm" (a permutation) or "rep" (with repeats)
CASES = {
    "1x1": (1, 1, 1, 1, 0, 0, None, None, "all"),
    "1x70": (1, 70, 3, 20, 2, 0, None, "rep", "all"),
    "17x33": (17, 33, 32, 40, 7, 5, "rep", None, "mixed"),
    "64x64": (64, 64, 64, 64, 0, 0, None, None, None),
    "64x64s5": (64, 64, 3, 1, 5, 1, "perm", "perm", "mixed"),
    "65x130": (65, 130, 100, 20, 3, 28, "rep", "rep", "mixed"),
    "65x130none": (65, 130, 1, 1, 1, 0, None, None, "none"),
    "17x33wide": (17, 33, 256, 64, 2, 0, None, "perm", "all"),
    "130x1000": (130, 1000, 256, 40, 7, 0, None, None, "mixed"),
    "130x1000k0": (130, 1000, 64, 0, 0, 0, "perm", None, "all"),
    "130x1000s3": (130, 1000, 32, 64, 3, 3, None, "rep", "mixed"),
    "1x70k0": (1, 70, 64, 0, 1, 0, None, None, None),
}


class Sim:
    """the library under test, its pointer function and its device (the emulator works on CPU tensors)"""

    def __init__(self, lib, ptr, device):
        self.lib, self.ptr, self.device = lib, ptr, torch.device(device)
        self.engine = SimilarityEngine(lib, ptr)

    def t(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def table(self, a, ld_extra=0):
        """the table as a view of a wider buffer (ld = D + ld_extra), the rest filled with a value that must not be read"""
        if not ld_extra:
            return self.t(a)
        wide = np.full((a.shape[0], a.shape[1] + ld_extra), 1e30, dtype=np.float32)
        wide[:, : a.shape[1]] = a
        return self.t(wide)[:, : a.shape[1]]

    def search(self, p, **kw):
        res = self.engine.search(self.table(p["emb_q"], p["ld_extra"]), self.table(p["emb_c"], p["ld_extra"]), self.t(p["q_idx"]),
                                 self.t(p["c_idx"]), self.t(p["target"]), k=p["k"], normalize=p["normalize"], splits=p["splits"],
                                 **kw)
        return {key: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for key, v in res.items()}


# ------------------------------------------------------------------------------------------------------ the restatement
def selected(emb, idx, m):
    """(rows float64 [m, D], present bool [m]) of a table under an index list; rows outside the table are absent"""
    idx = np.arange(m) if idx is None else np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < emb.shape[0])
    rows = np.zeros((m, emb.shape[1]))
    rows[ok] = emb[idx[ok]].astype(np.float64)
    return rows, ok


def unit(rows):
    n = np.sqrt((rows * rows).sum(1, keepdims=True))
    return np.divide(rows, n, out=np.zeros_like(rows), where=n > 0)


def restate(p):
    """float64: dict(scores [mq, mc], q_ok, c_ok, target (checked), greater, equal_before, target_score, topk_col, topk_score)"""
    mq = len(p["q_idx"]) if p["q_idx"] is not None else p["emb_q"].shape[0]
    mc = len(p["c_idx"]) if p["c_idx"] is not None else p["emb_c"].shape[0]
    q, q_ok = selected(p["emb_q"], p["q_idx"], mq)
    c, c_ok = selected(p["emb_c"], p["c_idx"], mc)
    if p["normalize"]:
        q, c = unit(q), unit(c)
    s = q @ c.T
    t = np.full(mq, -1, dtype=np.int64) if p["target"] is None else np.asarray(p["target"], dtype=np.int64).copy()
    t[(t < -1) | (t >= mc)] = -1
    t[~q_ok] = -1
    t[(t >= 0) & ~c_ok[np.maximum(t, 0)]] = -1
    k = p["k"]
    out = dict(scores=s, q_ok=q_ok, c_ok=c_ok, target=t, greater=np.full(mq, -1, np.int32), equal_before=np.full(mq, -1, np.int32),
               target_score=np.full(mq, np.nan), topk_col=np.full((mq, k), -1, np.int32), topk_score=np.full((mq, k), -np.inf))
    cols = np.arange(mc)
    for i in range(mq):
        if t[i] >= 0:
            st = s[i, t[i]]
            out["greater"][i] = int((c_ok & (s[i] > st)).sum())
            out["equal_before"][i] = int((c_ok & (s[i] == st) & (cols < t[i])).sum())
            out["target_score"][i] = st
        if k and q_ok[i]:
            live = cols[c_ok]
            order = live[np.lexsort((live, -s[i, live]))][:k]            # score descending, then column ascending
            out["topk_col"][i, : len(order)] = order
            out["topk_score"][i, : len(order)] = s[i, order]
    return out


# ------------------------------------------------------------------------------------------------------------ the cases
def _idx(kind, m, rows, rng):
    if kind is None:
        return None
    if kind == "perm":
        return rng.permutation(rows)[:m].astype(np.int32)
    return rng.randint(0, rows, m).astype(np.int32)                        # "rep": with repeats


def _targets(kind, mq, mc, rng):
    if kind is None:
        return None
    t = rng.randint(0, mc, mq).astype(np.int32)
    if kind == "none":
        t[:] = -1
    elif kind == "mixed":
        t[rng.rand(mq) < 0.3] = -1
        t[0] = -1 if mq > 1 else t[0]
    return t


@functools.lru_cache(maxsize=None)
def problem(name, tier):
    """the inputs of one case in one tier ("exact" / "norm") with their restatement, computed once and shared"""
    mq, mc, D, k, splits, ld_extra, qk, ck, tk = CASES[name]
    rng = np.random.RandomState(sorted(CASES).index(name) * 2 + (tier == "norm"))
    rows_q = mq if qk is None else mq + 7
    rows_c = mc if ck is None else mc + 5
    q_idx, c_idx = _idx(qk, mq, rows_q, rng), _idx(ck, mc, rows_c, rng)
    target = _targets(tk, mq, mc, rng)
    if tier == "exact":
        emb_q = rng.randint(-3, 4, (rows_q, D)).astype(np.float32)
        emb_c = rng.randint(-3, 4, (rows_c, D)).astype(np.float32)
    else:
        emb_q = rng.randn(rows_q, D).astype(np.float32)
        emb_c = rng.randn(rows_c, D).astype(np.float32)
        if target is not None:                                   # planted matches: the target's row is the query's plus noise
            for i in range(mq):
                if target[i] >= 0:
                    qr = i if q_idx is None else q_idx[i]
                    cr = target[i] if c_idx is None else c_idx[target[i]]
                    emb_c[cr] = emb_q[qr] + rng.uniform(0.3, 1.5) * rng.randn(D).astype(np.float32)
    p = dict(emb_q=emb_q, emb_c=emb_c, q_idx=q_idx, c_idx=c_idx, target=target, k=k, splits=splits, ld_extra=ld_extra,
             normalize=int(tier == "norm"))
    p["ref"] = restate(p)
    return p


# ----------------------------------------------------------------------------------------------------------- the checks
def assert_exact(got, ref):
    assert np.array_equal(got["greater"], ref["greater"])
    assert np.array_equal(got["equal_before"], ref["equal_before"])
    assert np.array_equal(got["target_score"], ref["target_score"].astype(np.float32), equal_nan=True)
    assert np.array_equal(got["topk_col"], ref["topk_col"])
    assert np.array_equal(got["topk_score"], ref["topk_score"].astype(np.float32))


def assert_hits_agree(got, ref):
    """Recall from the counts against the lists: a query with a target is a hit at k exactly when its target is listed"""
    k = got["k"]
    if k == 0:
        return
    for i in np.nonzero(ref["target"] >= 0)[0]:
        hit = got["greater"][i] + got["equal_before"][i] < k
        assert hit == (ref["target"][i] in got["topk_col"][i]), i


def assert_within_delta(got, ref):
    s, t, k = ref["scores"], ref["target"], got["k"]
    mq, mc = s.shape
    live = np.nonzero(ref["c_ok"])[0]
    for i in range(mq):
        if t[i] >= 0:
            st = s[i, t[i]]
            others = live[live != t[i]]
            lo, hi = int((s[i, live] > st + DELTA).sum()), int((s[i, others] > st - DELTA).sum())
            assert lo <= got["greater"][i] <= hi, (i, lo, got["greater"][i], hi)
            assert 0 <= got["equal_before"][i] <= int((np.abs(s[i, others] - st) <= DELTA).sum())
            assert abs(float(got["target_score"][i]) - st) <= DELTA, i
        else:
            assert got["greater"][i] == -1 and got["equal_before"][i] == -1 and np.isnan(got["target_score"][i])
        if k == 0:
            continue
        n = min(k, len(live)) if ref["q_ok"][i] else 0
        col, sc = got["topk_col"][i], got["topk_score"][i]
        assert (col[n:] == -1).all() and np.isneginf(sc[n:]).all()
        assert len(set(col[:n].tolist())) == n and np.isin(col[:n], live).all()
        assert (np.abs(sc[:n] - s[i, col[:n]]) <= DELTA).all(), i
        for a in range(n - 1):                                   # the list's own order: score descending, then column ascending
            assert sc[a] > sc[a + 1] or (sc[a] == sc[a + 1] and col[a] < col[a + 1]), (i, a)
        if n:
            kth = np.sort(s[i, live])[::-1][n - 1]
            must = live[s[i, live] > kth + 2 * DELTA]
            assert np.isin(must, col[:n]).all(), i
            assert (s[i, col[:n]] >= kth - 2 * DELTA).all(), i


def check_case(S, name, tier):
    p = problem(name, tier)
    got = S.search(p)
    assert got["status"][0] == 0
    if tier == "exact":
        assert_exact(got, p["ref"])
    else:
        assert_within_delta(got, p["ref"])
    assert_hits_agree(got, p["ref"])


def check_duplicate_rows(S):
    """the target's row listed three more times, at lower and higher columns and in other splits: the copies tie bitwise"""
    rng = np.random.RandomState(77)
    D, mc, k = 100, 40, 20
    emb_q = rng.randn(6, D).astype(np.float32)
    emb_c = rng.randn(50, D).astype(np.float32)
    emb_c[44] = emb_q[0]                                         # query 0's match is an exact copy: the best score there is
    emb_c[45] = emb_q[3] + 0.5 * rng.randn(D).astype(np.float32)
    c_idx = rng.randint(0, 44, mc).astype(np.int32)
    c_idx[[3, 10, 20, 30]] = 44                                  # splits = 3 searches the columns 0-15, 16-31, 32-39 apart
    c_idx[[18, 19, 35]] = 45
    target = np.array([20, -1, 5, 19, 7, -1], dtype=np.int32)
    p = dict(emb_q=emb_q, emb_c=emb_c, q_idx=None, c_idx=c_idx, target=target, k=k, splits=3, ld_extra=0, normalize=1)
    got, ref = S.search(p), restate(p)
    assert got["status"][0] == 0
    assert got["greater"][0] == 0 and got["equal_before"][0] == 2
    assert got["topk_col"][0, :4].tolist() == [3, 10, 20, 30]
    assert len(set(got["topk_score"][0, :4].view(np.int32).tolist())) == 1
    assert got["topk_score"][0, 0].view(np.int32) == got["target_score"][0].view(np.int32)
    assert got["equal_before"][3] == 1                           # column 18 before the target 19; 35 comes after it
    where = [got["topk_col"][3].tolist().index(c) for c in (18, 19, 35)]
    assert where == sorted(where) and where[2] - where[0] == 2
    assert len(set(got["topk_score"][3, where].view(np.int32).tolist())) == 1
    assert_within_delta(got, ref)
    assert_hits_agree(got, ref)


def check_zero_row(S):
    p = dict(problem("17x33", "norm"))
    p["emb_c"] = p["emb_c"].copy()
    p["emb_c"][4] = 0.0
    got, ref = S.search(p), restate(p)
    assert got["status"][0] == _cabi.STATUS_SIM_ZERO_ROW
    assert_within_delta(got, ref)                                # the zero row scores 0 against everything
    res = dict(status=torch.from_numpy(got["status"]))
    with pytest.raises(RuntimeError, match="norm 0"):
        S.engine.check_status(res)
    S.engine.check_status(res, allow_zero_rows=True)
    p["normalize"] = 0                                           # raw dot products: a zero row is nothing special
    assert S.search(p)["status"][0] == 0


def check_bad_index(S):
    """a query index, a candidate index and two targets out of range: one status bit, the other rows as if the bad ones were
    absent (restate() treats them so)"""
    p = dict(problem("65x130", "exact"))
    p["q_idx"], p["c_idx"], p["target"] = p["q_idx"].copy(), p["c_idx"].copy(), p["target"].copy()
    p["q_idx"][5] = p["emb_q"].shape[0]
    p["q_idx"][64] = -1
    p["c_idx"][77] = p["emb_c"].shape[0] + 3
    p["c_idx"][0] = -2
    p["target"][9], p["target"][10], p["target"][11] = 130, -2, 77
    got, ref = S.search(p), restate(p)
    assert got["status"][0] == _cabi.STATUS_SIM_BAD_INDEX
    assert ref["target"][[5, 64, 9, 10, 11]].tolist() == [-1] * 5 and (got["topk_col"][[5, 64]] == -1).all()
    assert not np.isin([0, 77], got["topk_col"]).any()
    assert_exact(got, ref)
    with pytest.raises(RuntimeError, match="outside its table"):
        S.engine.check_status(dict(status=torch.from_numpy(got["status"])))


def raw_call(S, **over):
    """gcc_sim_search through the bare C ABI on a small valid problem with members overridden; -> (rc, error text, outputs)"""
    mq, mc, D, k = 5, 9, 8, 3
    rng = np.random.RandomState(1)
    bufs = dict(emb_q=S.t(rng.randn(mq, D).astype(np.float32)), emb_c=S.t(rng.randn(mc, D).astype(np.float32)),
                greater=S.t(np.full(mq, -7, np.int32)), equal_before=S.t(np.full(mq, -7, np.int32)),
                target_score=S.t(np.full(mq, -7, np.float32)), topk_col=S.t(np.full((mq, 64), -7, np.int32)),
                topk_score=S.t(np.full((mq, 64), -7, np.float32)), target=S.t(np.zeros(mq, np.int32)),
                status=S.t(np.zeros(1, np.int32)), ws=S.t(np.zeros(1 << 20, np.uint8)))
    a = _cabi.GccSimArgs()
    a.emb_q, a.rows_q, a.ld_q, a.emb_c, a.rows_c, a.ld_c = S.ptr(bufs["emb_q"]), mq, D, S.ptr(bufs["emb_c"]), mc, D
    a.target = S.ptr(bufs["target"])
    a.mq, a.mc, a.D, a.k, a.normalize, a.splits = mq, mc, D, k, 1, 0
    for name in ("greater", "equal_before", "target_score", "topk_col", "topk_score"):
        setattr(a, name, S.ptr(bufs[name]))
    ws_bytes, status, ws = bufs["ws"].numel(), S.ptr(bufs["status"]), S.ptr(bufs["ws"])
    for key, v in over.items():
        if key == "workspace_bytes":
            ws_bytes = v
        elif key == "status":
            status = v
        elif key == "workspace":
            ws = v
        else:
            setattr(a, key, v)
    rc = S.lib.gcc_sim_search(ctypes.byref(a), ws, ws_bytes, status, None)
    if S.device.type == "cuda":
        torch.cuda.synchronize()
    outs = {n: bufs[n].cpu().numpy() for n in ("greater", "equal_before", "target_score", "topk_col", "topk_score", "status")}
    return rc, S.lib.gcc_last_error().decode(), outs


def check_refusals(S):
    rc, _, outs = raw_call(S)
    assert rc == 0 and (outs["greater"] >= 0).all() and (outs["topk_col"].reshape(-1)[:15] >= 0).all()       # the problem itself is served
    refused = [(dict(D=0), "D 0 outside"), (dict(D=257, ld_q=257, ld_c=257), "D 257 outside"), (dict(k=65), "k 65 outside"),
               (dict(k=-1), "k -1 outside"), (dict(splits=65), "splits 65 outside"), (dict(splits=-1), "splits -1 outside"),
               (dict(mq=-1), "mq -1"), (dict(emb_q=None), "emb_q is NULL"), (dict(emb_c=None), "emb_c is NULL"),
               (dict(ld_q=7), "ld_q 7"), (dict(mc=10), "mc 10 beyond"), (dict(workspace_bytes=64), "workspace_bytes 64"),
               (dict(workspace=None), "workspace_bytes 0"), (dict(status=None), "status is NULL")]
    for over, text in refused:
        rc, err, outs = raw_call(S, **over)
        assert rc < 0 and text in err and err.startswith("gcc_sim_search:"), (over, rc, err)
        for name, v in outs.items():                             # nothing was launched: every output keeps its fill
            assert (v == (0 if name == "status" else -7)).all(), (over, name)
    for over in (dict(mq=0), dict(mc=0)):                        # an empty side is served: no launch, outputs untouched
        rc, _, outs = raw_call(S, **over)
        assert rc == 0 and all((v == (0 if name == "status" else -7)).all() for name, v in outs.items()), over
    assert S.lib.gcc_sim_workspace_bytes(5, 9, 300, 3, 0) < 0 and "D 300" in S.lib.gcc_last_error().decode()
    assert S.lib.gcc_sim_workspace_bytes(5, 9, 8, 3, 0) <= 1 << 20


def check_engine(S):
    """the Python surface: recall_at_k from the counts, empty sides, argument errors by name"""
    p = problem("130x1000", "exact")
    res = S.engine.search(S.table(p["emb_q"]), S.table(p["emb_c"]), target=S.t(p["target"]), k=p["k"], normalize=False, splits=2)
    ref = p["ref"]
    have = ref["target"] >= 0
    before = (ref["greater"] + ref["equal_before"])[have]
    assert S.engine.recall_at_k(res, (1, 20, 40)) == {kk: float((before < kk).sum()) / have.sum() for kk in (1, 20, 40)}
    S.engine.check_status(res)
    empty = S.engine.search(S.t(np.zeros((0, 8), np.float32)), S.table(p["emb_c"][:, :8].copy()), k=4)
    assert empty["topk_col"].shape == (0, 4) and np.isnan(S.engine.recall_at_k(empty, (20,))[20])
    none = S.engine.search(S.table(p["emb_q"]), S.t(np.zeros((0, 256), np.float32)), target=None, k=4)
    assert (none["topk_col"].cpu().numpy() == -1).all() and (none["greater"].cpu().numpy() == -1).all()
    with pytest.raises(ValueError, match="emb_q has 256 columns, emb_c 8"):
        S.engine.search(S.table(p["emb_q"]), S.table(p["emb_c"][:, :8].copy()))
    with pytest.raises(ValueError, match="target has 3 entries"):
        S.engine.search(S.table(p["emb_q"]), S.table(p["emb_c"]), target=S.t(np.zeros(3, np.int32)))
    with pytest.raises(RuntimeError, match="k 65 outside"):
        S.engine.search(S.table(p["emb_q"]), S.table(p["emb_c"]), k=65)
