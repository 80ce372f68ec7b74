"""The ProNE kernels (gcc_amd/csrc/prone.hip) against the reference's own runs (tests/golden/prone_*.npz), scipy and NumPy, shared
by the emulator tier (tests/test_prone_emu.py) and the GPU tier (tests/test_prone_gpu.py): the same cases and checks; only the
library, the pointer function and the device differ.

Tolerances.  Whole embedding: after per-column sign alignment, max|emb - ref_lu| <= 16 x the largest mutual distance among the
three reference runs of the fixture (LU, QR, gesvd): they all take a LAPACK SVD of the factor, the device squares the factor's
condition number in its Gram matrices.  Products: every entry within deg_max 2^-52 sum|terms| of scipy's (reordering only), an
entry without terms exactly zero.  Orthonormalisation: |Q^T Q - I| <= 1e-13, and |Q R2 R1 - Y| <= 8 k 2^-52 (|Q| |R2| |R1|) entry
by entry (two triangular solves and one product of factors, each within k 2^-52 of its operands' absolute product).  Node terms:
4 ulp of NumPy's."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gcc_amd import _cabi
from gcc_amd.prone import ProNEEngine
from tests import prone_reference as R

EPS = 2.0 ** -52
SPLIT_CHUNK = 64                                   # the hub's 297 neighbours: 4 parts of 64 and one of 41


class Pr:
    """the library under test, its pointer function and its device (the emulator works on CPU tensors)"""

    def __init__(self, lib, ptr, device):
        self.lib, self.ptr, self.device = lib, ptr, torch.device(device)
        self.engine = ProNEEngine(lib, ptr, device)

    def t(self, a, dtype=None):
        x = torch.from_numpy(np.ascontiguousarray(a))
        return (x if dtype is None else x.to(dtype)).to(self.device)

    def embed(self, fx, **kw):
        kw.setdefault("omega", fx["omega"])
        res = self.engine.embed(fx["row_ptr"], fx["col_idx"], fx["d"], **kw)
        return {k: v.cpu().numpy() for k, v in res.items()}

    def stage(self, name, row_ptr, col_idx, d, chunk=0, **members):
        """one stage call on fresh arguments -> status word; ``members``: tensors (their addresses) or plain numbers"""
        a, keep, _ = self.engine.graph_args(row_ptr, col_idx, d, chunk)
        for key, v in members.items():
            setattr(a, key, self.ptr(v) if isinstance(v, torch.Tensor) else v)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.engine.call(name, a, status)
        return int(status.cpu()[0])


def check_parity(pr, name):
    fx = R.fixture(name)
    out = pr.embed(fx, seed=fx["seed"])
    assert int(out["status"][0]) == 0
    emb = out["emb"]
    dist = float(np.abs(R.align(emb, fx["emb_lu"]) - fx["emb_lu"]).max())
    print(f"prone parity {name}: max|emb - lu| {dist:.3g} = {dist / fx['variant_distance']:.3g} x the variants' {fx['variant_distance']:.3g}")
    assert dist <= R.VARIANT_FACTOR * fx["variant_distance"]
    assert np.array_equal(out["emb32"], emb.astype(np.float32))
    isolated = np.diff(fx["row_ptr"]) == 0
    assert not emb[isolated].any() and not out["emb32"][isolated].any()
    assert np.all(np.diff(out["sigma"]) <= 0) and np.all(out["sigma"] > 0)
    # the sign rule: per column the entry of largest magnitude is positive in the decomposition's U; a row's scale is positive,
    # so the same holds for the entry of that row here whenever it is the column's largest of U (checked through the restatement)
    ref = R.embed_numpy(fx["row_ptr"], fx["col_idx"], fx["d"], omega=fx["omega"])["emb"]
    assert float(np.abs(emb - ref).max()) <= R.VARIANT_FACTOR * fx["variant_distance"]          # (no alignment: the signs are pinned)


def check_step_one(pr):
    """step = 1 returns the factorisation's rows (prone.py l.80)"""
    fx = R.fixture("n40d2")
    out = pr.embed(fx, step=1)
    ref = R.embed_numpy(fx["row_ptr"], fx["col_idx"], fx["d"], omega=fx["omega"], step=1)["emb"]
    assert int(out["status"][0]) == 0 and float(np.abs(out["emb"] - ref).max()) <= 1e-12


def check_node_terms(pr, name):
    fx = R.fixture(name)
    n = fx["n"]
    r, c = (torch.full((n,), 7.0, dtype=torch.float64, device=pr.device) for _ in range(2))
    assert pr.stage("gcc_prone_node_terms", fx["row_ptr"], fx["col_idx"], fx["d"], r=r, c=c) == 0
    deg, r_ref, c_ref = R.node_terms(fx["row_ptr"], fx["col_idx"])
    for got, ref in ((r.cpu().numpy(), r_ref), (c.cpu().numpy(), c_ref)):
        live = deg > 0
        assert np.all(np.abs(got[live] - ref[live]) <= 4 * np.spacing(np.abs(ref[live])))
        assert np.all(np.isposinf(got[~live]))


def _matrices(row_ptr, col_idx, mu):
    n = len(row_ptr) - 1
    deg, r, c = R.node_terms(row_ptr, col_idx)
    rows = np.repeat(np.arange(n), deg)
    ci, rp = col_idx.astype(np.int64), row_ptr.astype(np.int64)
    F = sp.csr_matrix((r[rows] + c[ci], ci, rp), shape=(n, n))
    Ft = sp.csr_matrix((r[ci] + c[rows], ci, rp), shape=(n, n))
    A = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    inv = 1.0 / (deg + 1.0)
    M = sp.diags((1.0 - inv) - mu) - sp.diags(inv) @ A
    return deg, r, c, F.tocsr(), Ft.tocsr(), sp.csr_matrix(M), sp.csr_matrix(sp.eye(n) + A)


def check_spmm(pr, name, k, chunk):
    """every mode and tail on the fixture's graph with k columns"""
    fx = R.fixture(name)
    n, rp, ci, mu, d = fx["n"], fx["row_ptr"], fx["col_idx"], 0.2, max(2, k - _cabi.PRONE_OVERSAMPLE)
    deg, r, c, F, Ft, M, A1 = _matrices(rp, ci, mu)
    deg_max = int(deg.max())
    rng = np.random.RandomState(k)
    x, z, w, conv0 = (rng.randn(n, k) for _ in range(4))
    alpha, beta = 0.37, -1.21
    r_t, c_t = pr.t(r), pr.t(c)                                    # (+inf at an isolated node: no product may read it)
    m, m_terms = M @ x, abs(M) @ np.abs(x)
    cases = [
        (_cabi.PRONE_MODE_F, 0, F @ x, abs(F) @ np.abs(x), None, None),
        (_cabi.PRONE_MODE_FT, 0, Ft @ x, abs(Ft) @ np.abs(x), None, None),
        (_cabi.PRONE_MODE_M, _cabi.PRONE_TAIL_NONE, m, m_terms, None, None),
        (_cabi.PRONE_MODE_A1, 0, A1 @ (x - z), A1 @ (np.abs(x) + np.abs(z)), None, None),
    ]
    y = 0.5 * m - z
    y_terms = 0.5 * m_terms + np.abs(z)
    cases.append((_cabi.PRONE_MODE_M, _cabi.PRONE_TAIL_HALF, y, y_terms, alpha * z + beta * y, np.abs(alpha * z) + abs(beta) * y_terms))
    y = (m - 2 * z) - w
    y_terms = m_terms + 2 * np.abs(z) + np.abs(w)
    cases.append((_cabi.PRONE_MODE_M, _cabi.PRONE_TAIL_CHEB, y, y_terms, conv0 + alpha * y, np.abs(conv0) + abs(alpha) * y_terms))
    for mode, tail, ref, terms, conv_ref, conv_terms in cases:
        out = torch.full((n, k), 3.0, dtype=torch.float64, device=pr.device)
        conv = pr.t(conv0.copy())
        status = pr.stage("gcc_prone_spmm", rp, ci, d, chunk, mode=mode, tail=tail, k=k, mu=mu, alpha=alpha, beta=beta, r=r_t, c=c_t,
                          x=pr.t(x), z=pr.t(z), w=pr.t(w), y=out, conv=conv)
        assert status == 0, (mode, tail)
        got = out.cpu().numpy()
        assert np.all(np.abs(got - ref) <= deg_max * EPS * terms), (mode, tail, float(np.abs(got - ref).max()))
        if mode in (_cabi.PRONE_MODE_F, _cabi.PRONE_MODE_FT):
            assert not got[deg == 0].any()                         # an empty row: exact zeros
        if conv_ref is not None:
            assert np.all(np.abs(conv.cpu().numpy() - conv_ref) <= deg_max * EPS * conv_terms), (mode, tail)
    # the chunk changes no bit
    if chunk:
        outs = []
        for ch in (chunk, 0):
            out = torch.empty((n, k), dtype=torch.float64, device=pr.device)
            pr.stage("gcc_prone_spmm", rp, ci, d, ch, mode=_cabi.PRONE_MODE_F, k=k, r=r_t, c=c_t, x=pr.t(x), y=out)
            outs.append(out.cpu().numpy())
        assert np.array_equal(outs[0], outs[1])


def check_orthonormalize(pr, n, k, seed):
    rng = np.random.RandomState(seed)
    y0 = rng.randn(n, k) @ (rng.randn(k, k) + 2 * np.eye(k)) * np.logspace(0, 2, k)      # columns over two decades
    d = max(2, k - _cabi.PRONE_OVERSAMPLE)
    row_ptr, col_idx = np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)      # (the graph takes no part)
    y, rfac = pr.t(y0.copy()), torch.zeros((2, k, k), dtype=torch.float64, device=pr.device)
    assert pr.stage("gcc_prone_orthonormalize", row_ptr, col_idx, d, k=k, y=y, rfac=rfac) == 0
    q, (r1, r2) = y.cpu().numpy(), rfac.cpu().numpy()
    assert float(np.abs(q.T @ q - np.eye(k)).max()) <= 1e-13
    assert np.all(np.tril(r1, -1) == 0) and np.all(np.tril(r2, -1) == 0)
    assert np.all(np.abs(q @ r2 @ r1 - y0) <= 8 * k * EPS * (np.abs(q) @ np.abs(r2) @ np.abs(r1)))


def check_bits(pr, name, chunks=(0, 32, SPLIT_CHUNK)):
    fx = R.fixture(name)
    first = pr.embed(fx)
    for chunk in chunks:
        again = pr.embed(fx, chunk=chunk)
        assert int(first["status"][0]) == 0 and int(again["status"][0]) == 0
        for key in ("emb", "emb32", "sigma2"):
            assert np.array_equal(first[key], again[key]), (chunk, key)


def star(n):
    row_ptr = np.concatenate([[0, n - 1], n - 1 + np.arange(1, n)]).astype(np.int32)
    col_idx = np.concatenate([np.arange(1, n), np.zeros(n - 1)]).astype(np.int32)
    return row_ptr, col_idx


def check_status_bits(pr):
    # a star's F has rank 2: the range finder of width 12 loses rank, and nothing but zeros comes out
    row_ptr, col_idx = star(40)
    res = pr.engine.embed(row_ptr, col_idx, 2, seed=1)
    assert int(res["status"].cpu()[0]) & _cabi.STATUS_PRONE_RANK
    assert np.isfinite(res["emb"].cpu().numpy()).all() and np.isfinite(res["emb32"].cpu().numpy()).all()
    with pytest.raises(RuntimeError, match="lost rank"):
        pr.engine.check_status(res)
    # a repeated entry in two rows (a multigraph parent)
    fx = R.fixture("n40d2")
    rp, ci = fx["row_ptr"].astype(np.int64), fx["col_idx"]
    u, v = 0, int(ci[0])
    at_u, at_v = int(rp[u]), int(rp[v] + np.searchsorted(ci[rp[v]:rp[v + 1]], u))
    first, second = sorted([(at_u, v), (at_v, u)])
    ci2 = np.insert(np.insert(ci, second[0], second[1]), first[0], first[1])
    bump = np.zeros(len(rp), dtype=np.int64)
    bump[u + 1:] += 1
    bump[v + 1:] += 1
    res = pr.engine.embed((rp + bump).astype(np.int32), ci2, 2, seed=1)
    assert int(res["status"].cpu()[0]) & _cabi.STATUS_PRONE_DUPLICATE
    with pytest.raises(RuntimeError, match="repeated entry"):
        pr.engine.check_status(res)
    # parts of 32 neighbours on a graph whose rows mostly have more: 2 nnz / GCC_PRONE_CHUNK + 64 parts do not hold them
    wide = R.fixture("n120d64")
    res = pr.engine.embed(wide["row_ptr"], wide["col_idx"], 2, chunk=32)
    assert int(res["status"].cpu()[0]) & _cabi.STATUS_PRONE_SPLIT_FULL and not res["emb"].cpu().numpy().any()
    with pytest.raises(RuntimeError, match="do not fit the workspace"):
        pr.engine.check_status(res)
    # an unsorted row and a column out of range: reported, nothing read out of bounds
    bad = ci.copy()
    at = int(rp[np.argmax(np.diff(rp))])
    bad[[at, at + 1]] = bad[[at + 1, at]]
    assert int(pr.engine.embed(fx["row_ptr"], bad, 2)["status"].cpu()[0]) & _cabi.STATUS_PRONE_BAD_CSR
    bad = ci.copy()
    bad[5] = fx["n"]
    res = pr.engine.embed(fx["row_ptr"], bad, 2)
    assert int(res["status"].cpu()[0]) & _cabi.STATUS_PRONE_BAD_CSR and not res["emb"].cpu().numpy().any()


def check_refusals(pr):
    fx = R.fixture("n40d2")
    rp, ci = fx["row_ptr"], fx["col_idx"]
    with pytest.raises(RuntimeError, match=r"n 40 is less than d \+ 10"):
        pr.engine.embed(rp, ci, 31)
    with pytest.raises(RuntimeError, match="GCC_PRONE_MAX_DIM"):
        pr.engine.embed(rp, ci, 65)
    with pytest.raises(RuntimeError, match="chunk 48"):
        pr.engine.embed(rp, ci, 2, chunk=48)
    with pytest.raises((RuntimeError, ValueError), match="step"):
        pr.engine.embed(rp, ci, 2, step=0)
    a, keep, n = pr.engine.graph_args(rp, ci, 2)
    status = torch.zeros(1, dtype=torch.int32, device=pr.device)
    with pytest.raises(RuntimeError, match="workspace_bytes 64 is less than gcc_prone_workspace_bytes"):
        pr.engine.call("gcc_prone_node_terms", a, status, workspace_bytes=64)
    a.step = 5
    with pytest.raises(RuntimeError, match="gcc_prone_embed.*omega is NULL"):
        pr.engine.call("gcc_prone_embed", a, status)
    a.k, a.mode = 12, _cabi.PRONE_MODE_F
    with pytest.raises(RuntimeError, match="gcc_prone_spmm.*x is NULL"):
        pr.engine.call("gcc_prone_spmm", a, status)
    a.k = 13
    with pytest.raises(RuntimeError, match="k 13 outside"):
        pr.engine.call("gcc_prone_orthonormalize", a, status)
    a.row_ptr = None
    with pytest.raises(RuntimeError, match="row_ptr is NULL"):
        pr.engine.call("gcc_prone_node_terms", a, status)
    assert pr.lib.gcc_prone_workspace_bytes(2 ** 31, 10, 2) < 0 and b"int32" in pr.lib.gcc_last_error()
    assert int(status.cpu()[0]) == 0                               # (nothing was launched)


def check_device_graph(pr):
    """the CSR of a DeviceGraph is served as it lies on the device; a multigraph parent is refused by name"""
    fx = R.fixture("n40d2")

    class Graph:
        row_ptr, col_idx, multigraph = pr.t(fx["row_ptr"]), pr.t(fx["col_idx"]), False

    res = pr.engine.embed_graph(Graph, fx["d"], omega=fx["omega"])
    assert np.array_equal(res["emb"].cpu().numpy(), pr.embed(fx)["emb"])
    Graph.multigraph = True
    with pytest.raises(ValueError, match="multigraph=True"):
        pr.engine.embed_graph(Graph, fx["d"])


def check_cpu_tensor_refused(lib):
    fx = R.fixture("n40d2")
    eng = ProNEEngine(lib, _cabi.dev_ptr, "cpu")
    with pytest.raises(RuntimeError, match="device \\(HIP\\) tensors only"):
        eng.embed(torch.from_numpy(fx["row_ptr"]), torch.from_numpy(fx["col_idx"]), 2)
    with pytest.raises(RuntimeError, match="device \\(HIP\\) tensors only"):
        eng.embed(fx["row_ptr"], fx["col_idx"], 2)
    assert ctypes.sizeof(_cabi.GccProneArgs) % 8 == 0
