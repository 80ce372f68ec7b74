"""The sampler's tables from a CSR that is already on the device (gcc_graph_tables / gcc_graph_tables_hub_adj,
gcc_amd/csrc/graph_tables.hip): what ``gcc_amd.graph`` computes on the host at upload.

    summary   int64 [8]: the longest row, sum d, sum d^2, the rows of at least ``hub_degree`` entries, the status bits the call set,
              ``num_shards`` - (the lowest shard without weight); the ONE block the host reads
    seed_cdf  float64 [n]: per worker shard the cdf of d^0.75 (``seed_cdf_table``): never descending, ending in exactly 1.0, the
              same bits for any grid size and any two calls, within (n_s + 64) * 2^-53 of the exact cdf -- not NumPy's bits
    hub_index / hub_adj   exactly ``hub_tables``' (integers; the bitmap by integer atomic OR)

``sb_degree`` = float(sum d^2) / float(sum d) equals the host's value bit for bit while sum d^2 < 2^53.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _cabi
from ._engine import CabiEngine

SUMMARY_NAMES = ("max_degree", "sum_degree", "sum_degree_squared", "hubs", "status", "bad_shard")


def empty_shard_error(shard_off, n, bad_shard_word, num_shards):
    """``seed_cdf_table``'s message for the lowest shard without weight (summary[5] = num_shards - that shard)"""
    s = max(int(num_shards), 1) - int(bad_shard_word)
    bounds = [0, int(n)] if shard_off is None or len(shard_off) <= 2 else [int(x) for x in shard_off]
    return f"seed cdf: the nodes [{bounds[s]}, {bounds[s + 1]}) of a worker shard have no edges (total deg^0.75 weight 0.0)"


class GraphTablesEngine(CabiEngine):
    """C-ABI calls of the table build.  ``lib``/``ptr`` are injectable for the emulator tests only."""

    def __init__(self, lib=None, ptr=None, device="cuda:0"):
        super().__init__(lib, ptr, device)

    def _args(self, row_ptr, col_idx, n, nnz, shard_off, hub_degree, max_hub_bytes, grid):
        a = _cabi.GccGraphTablesArgs()
        a.row_ptr = self.ptr(row_ptr) if row_ptr is not None else None
        a.col_idx = self.ptr(col_idx) if col_idx is not None and col_idx.numel() else None
        a.n, a.nnz = int(n), int(nnz)
        so = None
        if shard_off is not None:
            so = np.ascontiguousarray(shard_off, dtype=np.int64)           # (read by the host inside the call)
            a.shard_off, a.num_shards = so.ctypes.data, len(so) - 1
        a.hub_degree, a.max_hub_bytes, a.grid = int(hub_degree), int(max_hub_bytes), int(grid)
        return a, so

    def tables_into(self, row_ptr, n, nnz, summary, seed_cdf, hub_index, status, shard_off=None, hub_degree=0, grid=0,
                    workspace_bytes=None, num_shards=None):
        """The bare first call: ``row_ptr`` int32 [n + 1] where the kernels run, the outputs as the caller allocated them
        (``summary`` int64 [8], ``seed_cdf`` float64 [n], ``hub_index`` int32 [n] or None, ``status`` zeroed int32 [1]);
        ``shard_off``: host integers [S + 1] or None.  Enqueued on torch's current stream; nothing is read back."""
        a, keep = self._args(row_ptr, None, n, nnz, shard_off, hub_degree, 0, grid)
        if num_shards is not None:
            a.num_shards = int(num_shards)
        a.summary = self.ptr(summary) if summary is not None else None
        a.seed_cdf = self.ptr(seed_cdf) if seed_cdf is not None else None
        a.hub_index = self.ptr(hub_index) if hub_index is not None else None
        nbytes = _cabi.size_query(self.lib, "gcc_graph_tables_workspace_bytes", int(n), max(int(a.num_shards), 0))
        self.invoke("gcc_graph_tables", a, self.workspace(nbytes, status.device), status, workspace_bytes)
        del keep

    def hub_adj_into(self, row_ptr, col_idx, n, nnz, hub_index, hub_adj, num_hubs, hub_words, status, max_hub_bytes=0, grid=0):
        """The bare second call: ``hub_adj`` [num_hubs, hub_words] (32-bit words) is zeroed and filled from ``hub_index``."""
        a, _ = self._args(row_ptr, col_idx, n, nnz, None, 0, max_hub_bytes, grid)
        a.hub_index = self.ptr(hub_index) if hub_index is not None else None
        a.hub_adj = self.ptr(hub_adj) if hub_adj is not None else None
        a.num_hubs, a.hub_words = int(num_hubs), int(hub_words)
        self.invoke("gcc_graph_tables_hub_adj", a, self.workspace(256, status.device), status)

    def tables(self, row_ptr, col_idx, shard_off=None, hub_degree=_cabi.GRAPH_TABLES_HUB_DEGREE, max_hub_bytes=1 << 30, hub_table=True, grid=0):
        """row_ptr [n + 1], col_idx [nnz] (int32 device tensors, or arrays that are uploaded) -> dict(max_degree, sum_degree,
        sum_degree_squared, hubs, sb_degree (host numbers), seed_cdf (device float64 [n]), hub_index (device int32 [n]) and hub_adj
        (device int32 [H, words]) or None for both -- no hubs, a bitmap above ``max_hub_bytes``, or ``hub_table=False`` --, status).
        One host read: the summary.  A shard without weight raises ``seed_cdf_table``'s ValueError."""
        self.require_device(self.device)
        rp, ci = self.put(row_ptr, torch.int32), self.put(col_idx, torch.int32)
        self.require_device(rp)
        n, nnz, dev = int(rp.numel()) - 1, int(ci.numel()), rp.device
        so = None if shard_off is None or len(shard_off) <= 2 else [int(x) for x in shard_off]
        out = dict(seed_cdf=torch.empty(max(n, 0), dtype=torch.float64, device=dev), hub_index=None, hub_adj=None,
                   status=torch.zeros(1, dtype=torch.int32, device=dev))
        summary = torch.zeros(_cabi.GRAPH_TABLES_SUMMARY_WORDS, dtype=torch.int64, device=dev)
        index = torch.empty(n, dtype=torch.int32, device=dev) if hub_table and n > 0 else None
        self.tables_into(rp, n, nnz, summary, out["seed_cdf"], index, out["status"], so, hub_degree, grid)
        sm = [int(x) for x in summary.cpu()]
        if sm[4] & _cabi.STATUS_GRAPH_TABLES_EMPTY_SHARD:
            raise ValueError(empty_shard_error(so, n, sm[5], len(so) - 1 if so else 1))
        out.update(max_degree=sm[0], sum_degree=sm[1], sum_degree_squared=sm[2], hubs=sm[3], sb_degree=float(sm[2]) / float(sm[1]) if sm[1] else 0.0)
        H = sm[3]
        words = (H + 31) // 32
        if index is not None and H > 0 and H * words * 4 <= max_hub_bytes:
            adj = torch.empty((H, words), dtype=torch.int32, device=dev)
            self.hub_adj_into(rp, ci, n, nnz, index, adj, H, words, out["status"], max_hub_bytes, grid)
            out["hub_index"], out["hub_adj"] = index, adj
        return out
