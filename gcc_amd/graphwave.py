"""GraphWave node embeddings of a parent graph on the device (gcc_graphwave_*, gcc_amd/csrc/graphwave.hip): the second baseline the
reference's node classification and similarity search compare the pre-trained encoder against (gcc/models/emb/graphwave.py,
``--model graphwave``), as the reference calls it: automatic scales, the Chebyshev approximation of order 30, two filters,
time points on [0, 100].

The graph is an undirected one as symmetric CSR in node-id order with sorted rows and no self loops; a repeated entry is a
parallel edge and counts (gcc_amd.ingest.multigraph_csr), so the multigraph similarity-search networks are served.  With ``n``
the number of node ids that have an edge and ``T = d // 4``:

    M      = -D^-1/2 A D^-1/2                                   (L - I; 1 / sqrt(deg) is 0 for a node id without an edge)
    tau    = linspace(-log(0.95) sqrt(n / 2), -log(0.80) sqrt(n / 2), 2)
    H_i    = sum_{k = 0..30} c_k(tau_i) T_k(M)                  (Chebyshev polynomials; c_k: ``cheb_coefficients``)
    H_i    = where(H_i > 1e-4 / n, H_i, 0)
    chi[u, i 2T + 2j]     = (1 / n) sum_v cos(t_j H_i[v, u])    t = linspace(0, 100, T)
    chi[u, i 2T + 2j + 1] = (1 / n) sum_v sin(t_j H_i[v, u])

over the node ids v that have an edge; the row of an id without one is zero.  Scales, coefficients and time points are float64
NumPy values computed here and handed to the device in the call's arguments.  Two calls give the same bits, for every panel width.

Measured against the reference's own runs (tests/golden/graphwave_*.npz), as a multiple of each fixture's ``variant_distance``
(the bound is 16), on the MI355X and on the emulator alike: n40d4 exact (its yardstick is 0), n65d8 0.0095, n257d64 0.036, n300d16 0.11,
hub300d8 0.019, multi130d32 0.020, n40d256 0.011, task 0.17.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _cabi
from ._engine import CabiEngine

ORDER = _cabi.GRAPHWAVE_ORDER
SCALE = 100.0
THRESHOLD = 1e-4
ETA_MAX, ETA_MIN = 0.95, 0.80

STATUS_BITS = {_cabi.STATUS_GRAPHWAVE_BAD_CSR: "row_ptr / col_idx are not a sorted CSR without self loops over [0, n_rows)"}


def cheb_coefficients(tau, order=ORDER):
    """the ``order + 1`` Chebyshev coefficients of exp(-tau (x + 1)) on [-1, 1] by Chebyshev-Gauss quadrature at ``order`` nodes
    (the reference's ``compute_cheb_coeff_basis``) -> float64 [order + 1]"""
    xx = np.array([np.cos((2 * i - 1) * 1.0 / (2 * order) * math.pi) for i in range(1, order + 1)])
    basis = [np.ones(order), xx]
    for _ in range(order - 1):
        basis.append(2 * xx * basis[-1] - basis[-2])
    f = np.exp(-tau * (xx + 1))
    coeffs = 2.0 / order * (f * np.vstack(basis)).sum(1)
    coeffs[0] = coeffs[0] / 2
    return coeffs


def auto_taus(n):
    """the two scales the reference picks for a graph of ``n`` nodes (``approximate_lambda``: lambda_1 = 1 / n) -> float64 [2]"""
    l1 = 1.0 / n
    smax = -np.log(ETA_MIN) * np.sqrt(0.5 / l1)
    smin = -np.log(ETA_MAX) * np.sqrt(0.5 / l1)
    return np.linspace(smin, smax, 2)


def time_points(d):
    """-> float64 [d // 4] on [0, SCALE]"""
    return np.linspace(0, SCALE, d // 4)


def check_width(d):
    if d % 4 != 0 or not 4 <= d <= _cabi.GRAPHWAVE_MAX_DIM:
        raise ValueError(f"d {d}: a multiple of 4 in 4..{_cabi.GRAPHWAVE_MAX_DIM}")


def live_nodes(row_ptr):
    """the number of node ids that have an edge"""
    return int((np.diff(np.asarray(row_ptr, dtype=np.int64)) > 0).sum())


def heat_numpy(row_ptr, col_idx):
    """-> (live [n_rows] bool, the two heat matrices before the threshold over the live nodes float64 [2, n, n], the threshold)"""
    import scipy.sparse as sp

    row_ptr, col_idx = np.asarray(row_ptr, dtype=np.int64), np.asarray(col_idx, dtype=np.int64)
    n_rows = len(row_ptr) - 1
    live = np.diff(row_ptr) > 0
    n = int(live.sum())
    if not 2 <= n or n_rows > _cabi.GRAPHWAVE_MAX_NODES:
        raise ValueError(f"{n} nodes with an edge among {n_rows} ids: 2..{_cabi.GRAPHWAVE_MAX_NODES} are served")
    a = sp.csr_matrix((np.ones(len(col_idx)), col_idx, row_ptr), shape=(n_rows, n_rows))
    a.sum_duplicates()
    a = a[live][:, live]
    deg = np.asarray(a.sum(0)).reshape(-1)
    dinv = sp.diags(np.where(deg > 1e-10, 1.0 / np.sqrt(np.where(deg > 1e-10, deg, 1.0)), 0.0))
    m = sp.csr_matrix(-(dinv @ (a @ dinv)))
    coeff = [cheb_coefficients(tau) for tau in auto_taus(n)]
    x0, x1 = np.eye(n), m.toarray()
    heat = np.stack([c[0] * x0 + c[1] * x1 for c in coeff])
    for k in range(2, ORDER + 1):
        x0, x1 = x1, 2 * (m @ x1) - x0
        for i, c in enumerate(coeff):
            heat[i] += c[k] * x1
    return live, heat, THRESHOLD * 1.0 / n


def embed_numpy(row_ptr, col_idx, d):
    """The dense float64 restatement of what the device computes -> dict(chi float64 [n_rows, d], chi32, heat [2, n, n] after the
    threshold, live): what ``--device cpu`` serves."""
    check_width(d)
    live, heat, thr = heat_numpy(row_ptr, col_idx)
    n, T = heat.shape[1], d // 4
    heat = np.where(heat > thr, heat, 0.0)
    sig = np.zeros((n, d))
    for i in range(2):
        for j, t in enumerate(time_points(d)):
            arg = t * heat[i]
            sig[:, i * 2 * T + 2 * j] = np.cos(arg).sum(0) / n
            sig[:, i * 2 * T + 2 * j + 1] = np.sin(arg).sum(0) / n
    chi = np.zeros((len(live), d))
    chi[live] = sig
    return dict(chi=chi, chi32=chi.astype(np.float32), heat=heat, live=live)


class GraphWaveEngine(CabiEngine):
    """C-ABI calls of the embedding.  ``lib``/``ptr`` are injectable for the emulator tests only."""

    def __init__(self, lib=None, ptr=None, device="cuda:0"):
        super().__init__(lib, ptr, device)

    def graph_args(self, row_ptr, col_idx, d, width=0):
        """-> (args with the graph's members, scales' coefficients, time points and threshold filled, the tensors they point to)"""
        self.require_device(self.device)
        host_rp = row_ptr.cpu().numpy() if isinstance(row_ptr, torch.Tensor) else np.asarray(row_ptr)
        rp, ci = self.put(row_ptr, torch.int32), self.put(col_idx, torch.int32)
        n_rows, nnz = int(rp.numel()) - 1, int(ci.numel())
        a = _cabi.GccGraphwaveArgs()
        a.row_ptr, a.col_idx = self.ptr(rp), (self.ptr(ci) if nnz else None)
        a.n_rows, a.nnz, a.d, a.width = n_rows, nnz, int(d), int(width)
        n = live_nodes(host_rp) if n_rows >= 1 else 0
        if n >= 2:
            for i, tau in enumerate(auto_taus(n)):
                for k, c in enumerate(cheb_coefficients(tau)):
                    a.coeff[i][k] = c
        if d >= 4 and d // 4 <= _cabi.GRAPHWAVE_MAX_DIM // 4:
            for j, t in enumerate(time_points(int(d))):
                a.time_points[j] = t
        a.threshold = THRESHOLD
        return a, (rp, ci)

    def call(self, name, a, status, workspace_bytes=None):
        nbytes = _cabi.size_query(self.lib, "gcc_graphwave_workspace_bytes", int(a.n_rows), int(a.nnz), int(a.d), int(a.width))
        self.invoke(name, a, self.workspace(nbytes), status, workspace_bytes)

    def panel_width(self, n_rows, d, width=0):
        """the columns of one panel: ``width``, or the default the workspace is sized for"""
        return _cabi.size_query(self.lib, "gcc_graphwave_panel_width", int(n_rows), int(d), int(width))

    def embed(self, row_ptr, col_idx, d, width=0):
        """row_ptr [n_rows + 1], col_idx [nnz] (arrays or tensors) -> dict(chi float64 [n_rows, d], chi32 float32 [n_rows, d],
        status int32 [1]).  Everything is enqueued on torch's current stream; the results are not read back (a ``row_ptr`` that is a
        device tensor is read once, for the node count the scales depend on)."""
        a, keep = self.graph_args(row_ptr, col_idx, d, width)
        dev, n_rows = keep[0].device, int(a.n_rows)
        out = dict(chi=torch.empty((n_rows, d), dtype=torch.float64, device=dev),
                   chi32=torch.empty((n_rows, d), dtype=torch.float32, device=dev),
                   status=torch.zeros(1, dtype=torch.int32, device=dev))
        a.chi, a.chi32 = self.ptr(out["chi"]), self.ptr(out["chi32"])
        self.call("gcc_graphwave_embed", a, out["status"])
        return out

    def heat(self, row_ptr, col_idx, d, chunk=0, width=0):
        """the two thresholded heat panels of the source columns [chunk W, (chunk + 1) W) -> dict(heat float64 [2, n_rows, W],
        status); rows and columns of ids without an edge, and columns past n_rows, are zero (the stage tests)"""
        a, keep = self.graph_args(row_ptr, col_idx, d, width)
        dev, n_rows = keep[0].device, int(a.n_rows)
        w = self.panel_width(n_rows, d, width)
        out = dict(heat=torch.empty((2, n_rows, w), dtype=torch.float64, device=dev), status=torch.zeros(1, dtype=torch.int32, device=dev))
        a.heat, a.heat_chunk = self.ptr(out["heat"]), int(chunk)
        self.call("gcc_graphwave_heat", a, out["status"])
        return out

    def embed_graph(self, graph, d, **kw):
        """``embed`` on the CSR a gcc_amd.graph.DeviceGraph already holds on the device (a multigraph parent included)"""
        return self.embed(graph.row_ptr, graph.col_idx, d, **kw)

    @staticmethod
    def check_status(result):
        """Raises and names the bits of the call's status word (one host read)."""
        CabiEngine.raise_status(result, "gcc_graphwave", STATUS_BITS)
