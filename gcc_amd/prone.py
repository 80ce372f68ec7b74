"""ProNE node embeddings of a parent graph on the device (gcc_prone_*, gcc_amd/csrc/prone.hip): the baseline the reference's
node classification compares the pre-trained encoder against (gcc/models/emb/prone.py, ``--model prone``).

The graph is a simple undirected one as symmetric CSR in node-id order with sorted rows and no self loops, which is what
gcc_amd.ingest.read_edgelist returns.  The embedding is sklearn's ``randomized_svd(F, d, n_iter=5)`` of the factorised matrix
``F_ij = -log(deg_i) - log(neg_j)`` on A's pattern, then ``step`` terms of the Chebyshev-Gaussian propagation and the thin SVD of
its result, all in float64.  The reference draws its random test matrix from an unseeded generator; here Omega is an INPUT:
``np.random.RandomState(seed).normal(size=(n, d + 10))``, sklearn's own draw for that seed, unless the caller passes one.  The
signs of the singular vectors are pinned by sklearn's ``svd_flip`` rule in both decompositions (per column the entry of largest
magnitude is positive, ties to the lowest row).  Two calls on the same inputs give the same bits, for every chunk length.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _cabi
from ._engine import CabiEngine

STATUS_BITS = {_cabi.STATUS_PRONE_BAD_CSR: "row_ptr / col_idx are not a sorted CSR without self loops over [0, n)",
               _cabi.STATUS_PRONE_DUPLICATE: "a repeated entry in a row (a multigraph parent: the reference's nx.Graph has none)",
               _cabi.STATUS_PRONE_SPLIT_FULL: "the rows longer than this chunk do not fit the workspace",
               _cabi.STATUS_PRONE_RANK: "the range finder lost rank (a pivot of the orthonormalisation is not positive)",
               _cabi.STATUS_PRONE_SWEEPS: "the eigensolver stopped at its sweep limit",
               _cabi.STATUS_PRONE_SINGULAR: "a singular value is not above n eps sigma_1 (a rank-deficient factor)"}


def bessel_iv(order, x, terms=60):
    """the modified Bessel function of the first kind I_order(x) for an integer order >= 0, by its power series
    sum_m (x / 2)^(2 m + order) / (m! (m + order)!) (scipy.special.iv to the last bit or two for the |x| <= 2 used here)"""
    half = x / 2.0
    term = 1.0
    for i in range(1, order + 1):
        term *= half / i
    total = 0.0
    for m in range(terms):
        total += term
        term *= half * half / ((m + 1) * (m + 1 + order))
    return total


def draw_omega(n, d, seed):
    """sklearn's test matrix for ``randomized_svd(..., n_components=d, random_state=seed)``: float64 [n, d + 10]"""
    return np.random.RandomState(seed).normal(size=(n, d + _cabi.PRONE_OVERSAMPLE))


def flip_signs(u):
    """sklearn's svd_flip on the columns of u: the entry of largest magnitude positive, ties to the lowest row"""
    top = np.argmax(np.abs(u), axis=0)
    return u * np.where(u[top, np.arange(u.shape[1])] < 0, -1.0, 1.0)


def normalize_rows(u):
    norm = np.sqrt((u * u).sum(axis=1))
    return u / np.where(norm > 0, norm, 1.0)[:, None]


def node_terms(row_ptr, col_idx):
    """-> (deg, r, c) of prone.py l.56-76; an isolated node has r = c = +inf, which no product reads"""
    row_ptr, col_idx = np.asarray(row_ptr, dtype=np.int64), np.asarray(col_idx, dtype=np.int64)
    deg = np.diff(row_ptr)
    rows = np.repeat(np.arange(len(deg)), deg)
    with np.errstate(divide="ignore"):
        r = -np.log(deg.astype(np.float64))
        s = np.bincount(rows, weights=1.0 / deg[col_idx], minlength=len(deg))
        p = s ** 0.75
        c = -np.log(p / p.sum())
    return deg, r, c


def embed_numpy(row_ptr, col_idx, d, seed=0, omega=None, step=5, mu=0.2, theta=0.5):
    """The float64 restatement of what the device computes, stage by stage (scipy.sparse products, a QR normaliser, the two small
    symmetric eigenproblems by ``eigh`` of the Gram matrices, the sign rule) -> dict(emb, emb32, sigma, sigma0, fact): what
    ``--device cpu`` serves.  ``fact``: the factorisation's rows (``step`` = 1)."""
    import scipy.sparse as sp

    row_ptr, col_idx = np.asarray(row_ptr, dtype=np.int64), np.asarray(col_idx, dtype=np.int64)
    n, k = len(row_ptr) - 1, d + _cabi.PRONE_OVERSAMPLE
    if not 2 <= d <= _cabi.PRONE_MAX_DIM or n < k:
        raise ValueError(f"d {d} outside 2..{_cabi.PRONE_MAX_DIM}, or n {n} less than d + {_cabi.PRONE_OVERSAMPLE}")
    deg, r, c = node_terms(row_ptr, col_idx)
    rows = np.repeat(np.arange(n), deg)
    F = sp.csr_matrix((r[rows] + c[col_idx], col_idx, row_ptr), shape=(n, n))
    Ft = sp.csr_matrix((r[col_idx] + c[rows], col_idx, row_ptr), shape=(n, n))
    A = sp.csr_matrix((np.ones(len(col_idx)), col_idx, row_ptr), shape=(n, n))
    # (an isolated node's row of F Q is exactly zero; Householder QR would leave rounding there, which the row normalisation
    # would blow up to a unit row)
    orth = lambda y: np.linalg.qr(y)[0] * (deg > 0)[:, None]  # noqa: E731

    def top_pairs(g, count):
        lam, vec = np.linalg.eigh(g)
        order = np.argsort(-lam, kind="stable")[:count]
        return np.sqrt(np.maximum(lam[order], 0.0)), vec[:, order]

    q = np.asarray(omega, dtype=np.float64) if omega is not None else draw_omega(n, d, seed)
    for _ in range(5):
        q = orth(F @ q)
        q = orth(Ft @ q)
    q = orth(F @ q)
    bt = Ft @ q
    sigma0, uh = top_pairs(bt.T @ bt, d)
    fact = normalize_rows(flip_signs(q @ uh) * np.sqrt(sigma0))
    emb, sigma = fact, sigma0
    if step > 1:
        inv = 1.0 / (deg + 1.0)
        m_dot = lambda x: ((1.0 - inv) - mu)[:, None] * x - inv[:, None] * (A @ x)  # noqa: E731
        lx0, lx1 = fact, 0.5 * m_dot(m_dot(fact)) - fact
        conv = bessel_iv(0, theta) * lx0 + (-2.0 * bessel_iv(1, theta)) * lx1
        for i in range(2, step):
            lx2 = (m_dot(m_dot(lx1)) - 2.0 * lx1) - lx0
            conv = conv + (2.0 if i % 2 == 0 else -2.0) * bessel_iv(i, theta) * lx2
            lx0, lx1 = lx1, lx2
        diff = fact - conv
        mm = diff + A @ diff
        sigma, v = top_pairs(mm.T @ mm, d)
        emb = normalize_rows(flip_signs(mm @ v) / np.sqrt(sigma))
    return dict(emb=emb, emb32=emb.astype(np.float32), sigma=sigma, sigma0=sigma0, fact=fact)


class ProNEEngine(CabiEngine):
    """C-ABI calls of the embedding.  ``lib``/``ptr`` are injectable for the emulator tests only."""

    def __init__(self, lib=None, ptr=None, device="cuda:0"):
        super().__init__(lib, ptr, device)

    def graph_args(self, row_ptr, col_idx, d, chunk=0):
        """-> (args with the graph's members filled, the tensors they point to, n)"""
        rp, ci = self.put(row_ptr, torch.int32), self.put(col_idx, torch.int32)
        n, nnz = int(rp.numel()) - 1, int(ci.numel())
        a = _cabi.GccProneArgs()
        a.row_ptr, a.col_idx = self.ptr(rp), (self.ptr(ci) if nnz else None)
        a.n, a.nnz, a.d, a.chunk = n, nnz, int(d), int(chunk)
        return a, (rp, ci), n

    def call(self, name, a, status, workspace_bytes=None):
        nbytes = _cabi.size_query(self.lib, "gcc_prone_workspace_bytes", int(a.n), int(a.nnz), int(a.d))
        self.invoke(name, a, self.workspace(nbytes), status, workspace_bytes)

    def embed(self, row_ptr, col_idx, d, seed=0, omega=None, step=5, mu=0.2, theta=0.5, chunk=0):
        """row_ptr [n + 1], col_idx [nnz] (arrays or tensors); ``omega``: float64 [n, d + 10], default ``draw_omega(n, d, seed)``.
        -> dict(emb float64 [n, d], emb32 float32 [n, d], sigma float64 [d] (the last decomposition's singular values), sigma0
        (the factorisation's), status int32 [1]).  Everything is enqueued on torch's current stream; nothing is read back."""
        if isinstance(row_ptr, torch.Tensor):
            self.require_device(row_ptr)
        if not 1 <= int(step) <= _cabi.PRONE_MAX_STEP:
            raise ValueError(f"step {step} outside 1..{_cabi.PRONE_MAX_STEP}")
        a, keep, n = self.graph_args(row_ptr, col_idx, d, chunk)
        k = int(d) + _cabi.PRONE_OVERSAMPLE
        if omega is None:
            if n < k:                           # (the C call names it; no draw for a graph that is refused)
                omega = np.zeros((max(n, 0), k))
            else:
                omega = draw_omega(n, int(d), seed)
        om = self.put(omega, torch.float64)
        if tuple(om.shape) != (n, k):
            raise ValueError(f"omega must be [n, d + 10] = [{n}, {k}], got {tuple(om.shape)}")
        dev = om.device
        out = dict(emb=torch.empty((n, d), dtype=torch.float64, device=dev), emb32=torch.empty((n, d), dtype=torch.float32, device=dev),
                   sigma2=torch.empty((2, d), dtype=torch.float64, device=dev), status=torch.zeros(1, dtype=torch.int32, device=dev))
        a.step, a.mu = int(step), float(mu)
        for i in range(int(step)):
            a.bessel[i] = bessel_iv(i, float(theta))
        a.omega, a.emb, a.emb32, a.sigma = self.ptr(om), self.ptr(out["emb"]), self.ptr(out["emb32"]), self.ptr(out["sigma2"])
        self.call("gcc_prone_embed", a, out["status"])
        out["sigma0"], out["sigma"] = out["sigma2"][0], out["sigma2"][1 if int(step) > 1 else 0]
        return out

    def embed_graph(self, graph, d, **kw):
        """``embed`` on the CSR a gcc_amd.graph.DeviceGraph already holds on the device.  A multigraph parent is refused: the
        reference's ``nx.Graph`` collapses parallel edges, so ProNE is defined on the simple graph."""
        if getattr(graph, "multigraph", False):
            raise ValueError("ProNE takes a simple graph: DeviceGraph(multigraph=True) holds repeated row entries")
        return self.embed(graph.row_ptr, graph.col_idx, d, **kw)

    @staticmethod
    def check_status(result, allow_sweeps=False):
        """Raises and names the bits of the call's status word (one host read)."""
        CabiEngine.raise_status(result, "gcc_prone", STATUS_BITS, _cabi.STATUS_PRONE_SWEEPS if allow_sweeps else 0)
