"""Raw undirected edge lines -> the sampler's contract CSR on the device (gcc_graph_build, gcc_amd/csrc/graph_build.hip), and the
contract check on the device (gcc_graph_check).

The rule is the reference converter's (gcc/utils/x2dgl.py, ``yuxiao_kdd17_graph_to_dgl``):

    1. a line with u == v is dropped;
    2. both directions of every other line are inserted;
    3. repeats collapse to one entry (SciPy's ``tocsr`` sums them, DGL keeps one edge per non-zero);
    4. the nodes left without an entry are removed;
    5. the survivors are relabelled in ascending old-id order;
    6. rows are sorted ascending.

Integers only, so the result is a function of the set of lines: any order of the lines and any two calls give the same bits.
``build_csr_numpy`` restates the rule without a float; it is what ``--device cpu`` of ``python -m gcc_amd.x2dgl`` serves and what
every test compares the device against.

``counts`` (int64 [6]): nodes kept, entries written, u == v lines dropped, repeated directed slots dropped, nodes removed for
having no entry, the longest row.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _cabi
from ._engine import CabiEngine

COUNT_NAMES = ("nodes", "entries", "self_loop_lines", "duplicate_slots", "zero_degree_nodes", "max_degree")

BUILD_STATUS_BITS = {_cabi.STATUS_GRAPH_BUILD_BAD_ID: "a line names a node id outside [0, n): the line was ignored"}

# the check's bits in the order gcc_amd.graphgen.check_contract tests them, with its messages
STATUS_TEXT = {
    _cabi.STATUS_GRAPH_CHECK_SPAN: "row_ptr does not span col_idx",
    _cabi.STATUS_GRAPH_CHECK_ZERO_DEGREE: "zero-degree node: the reference removes them (x2dgl.py:61) and DGL's walker aborts on them",
    _cabi.STATUS_GRAPH_CHECK_RANGE: "col_idx out of range",
    _cabi.STATUS_GRAPH_CHECK_UNSORTED: "rows must be sorted ascending",
    _cabi.STATUS_GRAPH_CHECK_SELF_LOOP: "self loop present (x2dgl.py:41-42)",
    _cabi.STATUS_GRAPH_CHECK_DUPLICATE: "duplicate edge present (x2dgl.py:52-54)",
    _cabi.STATUS_GRAPH_CHECK_ASYMMETRIC: "graph is not symmetric (x2dgl.py:43-47)",
}
# where check_multigraph_contract words a violation differently
STATUS_TEXT_MULTIGRAPH = {
    **STATUS_TEXT,
    _cabi.STATUS_GRAPH_CHECK_UNSORTED: "rows must be sorted (non-decreasing: the copies of a parallel edge are adjacent)",
    _cabi.STATUS_GRAPH_CHECK_ASYMMETRIC: "graph is not symmetric with equal copy counts in both directions (x2dgl.py:43-47)",
}


def build_csr_numpy(pairs, n):
    """pairs [m, 2] (any integer type), n declared nodes -> dict(row_ptr int32 [kept + 1], col_idx int32 [entries], node_map int32
    [n], counts int64 [6], status int32 [1]) by the rule above, in int64 arithmetic throughout."""
    n = int(n)
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"n {n} outside 1..2^31 - 1: node ids are int32")
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if 2 * len(pairs) >= 2 ** 31:
        raise ValueError(f"m {len(pairs)}: 2 m must stay below 2^31, entry offsets are int32")
    u, v = pairs[:, 0], pairs[:, 1]
    bad = (u < 0) | (u >= n) | (v < 0) | (v >= n)
    loop = ~bad & (u == v)
    on = ~(bad | loop)
    u, v = u[on], v[on]
    key = np.unique(np.concatenate([u * n + v, v * n + u]))         # row-major (row, column), ascending: sorted rows
    rows, cols = key // n, key % n
    deg = np.bincount(rows, minlength=n)
    alive = deg > 0
    kept = int(alive.sum())
    node_map = np.where(alive, np.cumsum(alive) - 1, -1).astype(np.int32)
    row_ptr = np.zeros(kept + 1, dtype=np.int64)
    np.cumsum(deg[alive], out=row_ptr[1:])
    counts = np.array([kept, len(key), int(loop.sum()), 2 * int(on.sum()) - len(key), n - kept, int(deg.max()) if len(key) else 0],
                      dtype=np.int64)
    status = np.array([_cabi.STATUS_GRAPH_BUILD_BAD_ID if bad.any() else 0], dtype=np.int32)
    return dict(row_ptr=row_ptr.astype(np.int32), col_idx=node_map[cols].astype(np.int32), node_map=node_map, counts=counts, status=status)


def contract_error(status, multigraph=False):
    """the message gcc_amd.graphgen.check_contract (check_multigraph_contract) raises for the first violation among the bits of
    ``status``; None for 0"""
    for bit, text in (STATUS_TEXT_MULTIGRAPH if multigraph else STATUS_TEXT).items():
        if int(status) & bit:
            return text
    return None


class GraphBuildEngine(CabiEngine):
    """C-ABI calls of the build and of the check.  ``lib``/``ptr`` are injectable for the emulator tests only."""

    def __init__(self, lib=None, ptr=None, device="cuda:0"):
        super().__init__(lib, ptr, device)

    def build_into(self, pairs, n, row_ptr, col_idx, node_map, counts, status, workspace_bytes=None):
        """The bare call: ``pairs`` int32 [m, 2] where the kernels run, the outputs as the caller allocated them (``row_ptr`` of
        n + 1 words, ``col_idx`` of 2 m, ``node_map`` of n or None, ``counts`` int64 [6], ``status`` zeroed int32 [1]).  Enqueued on
        torch's current stream; nothing is read back."""
        m = int(pairs.numel()) // 2
        a = _cabi.GccGraphBuildArgs()
        a.pairs = self.ptr(pairs) if pairs is not None and m else None
        a.n, a.m = int(n), m
        a.row_ptr = self.ptr(row_ptr) if row_ptr is not None else None
        a.col_idx = self.ptr(col_idx) if col_idx is not None and col_idx.numel() else None
        a.node_map = self.ptr(node_map) if node_map is not None else None
        a.counts = self.ptr(counts) if counts is not None else None
        nbytes = _cabi.size_query(self.lib, "gcc_graph_build_workspace_bytes", int(n), m)
        self.invoke("gcc_graph_build", a, self.workspace(nbytes, status.device), status, workspace_bytes)

    def build(self, pairs, n):
        """pairs [m, 2] (an array, or an int32 tensor on the device), n declared nodes -> dict(row_ptr, col_idx (device int32,
        sliced to what was written), node_map (device int32 [n]), counts (int64 [6], on the host), status (device int32 [1])).
        One host read: ``counts``."""
        self.require_device(self.device)
        n = int(n)
        if not isinstance(pairs, torch.Tensor):
            pairs = np.asarray(pairs).reshape(-1, 2)
            if pairs.dtype != np.int32 and len(pairs) and (pairs.min() < -2 ** 31 or pairs.max() >= 2 ** 31):
                raise ValueError("node ids must fit int32")
        p = self.put(pairs, torch.int32).reshape(-1, 2)
        self.require_device(p)
        m, dev = int(p.shape[0]), p.device
        if not 1 <= n < 2 ** 31 or 2 * m >= 2 ** 31:
            _cabi.size_query(self.lib, "gcc_graph_build_workspace_bytes", n, m)       # (raises and names the size)
        out = dict(row_ptr=torch.empty(n + 1, dtype=torch.int32, device=dev), col_idx=torch.empty(2 * m, dtype=torch.int32, device=dev),
                   node_map=torch.empty(n, dtype=torch.int32, device=dev), counts=torch.zeros(6, dtype=torch.int64, device=dev),
                   status=torch.zeros(1, dtype=torch.int32, device=dev))
        self.build_into(p, n, out["row_ptr"], out["col_idx"], out["node_map"], out["counts"], out["status"])
        out["counts"] = out["counts"].cpu()
        kept, entries = int(out["counts"][0]), int(out["counts"][1])
        out["row_ptr"], out["col_idx"] = out["row_ptr"][: kept + 1], out["col_idx"][:entries]
        return out

    def check(self, row_ptr, col_idx, multigraph=False):
        """row_ptr [n + 1], col_idx [nnz] (arrays or device tensors) -> dict(status int32 [1], maxima int32 [2]: the longest row
        and the most copies of one entry in a row), both on the device; nothing is read back.  The reverse entries (and
        maxima[1]) are looked at only when every other test passed."""
        self.require_device(self.device)
        rp, ci = self.put(row_ptr, torch.int32), self.put(col_idx, torch.int32)
        self.require_device(rp)
        a = _cabi.GccGraphCheckArgs()
        a.row_ptr, a.col_idx = self.ptr(rp), (self.ptr(ci) if ci.numel() else None)
        a.n, a.nnz, a.multigraph = int(rp.numel()) - 1, int(ci.numel()), int(bool(multigraph))
        out = dict(status=torch.zeros(1, dtype=torch.int32, device=rp.device), maxima=torch.zeros(2, dtype=torch.int32, device=rp.device))
        a.maxima = self.ptr(out["maxima"])
        self.invoke("gcc_graph_check", a, self.workspace(256, rp.device), out["status"])
        return out

    def validate(self, row_ptr, col_idx, multigraph=False):
        """``check`` and one host read: raises ValueError with check_contract's message -> (max_degree, max_copies)"""
        res = self.check(row_ptr, col_idx, multigraph)
        text = contract_error(int(res["status"].cpu()[0]), multigraph)
        if text:
            raise ValueError(text)
        mx = res["maxima"].cpu()
        return int(mx[0]), int(mx[1])

    @staticmethod
    def check_status(result):
        """Raises and names the bits of a build's status word (one host read)."""
        CabiEngine.raise_status(result, "gcc_graph_build", BUILD_STATUS_BITS)
