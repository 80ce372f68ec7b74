"""Parent graph resident in HBM.

The reference keeps one DGLGraph copy per DataLoader worker process
(/root/reference/gcc/datasets/graph_dataset.py:23-30); here the CSR is uploaded
once per GPU and every kernel reads it in place.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _cabi
from .graphgen import check_contract, check_multigraph_contract


def seed_cdf_table(row_ptr: np.ndarray, shard_off=None) -> np.ndarray:
    """P(seed = v) ~ in_degree(v)^0.75 (graph_dataset.py:86-90) as the float64
    cdf numpy's ``choice(p=...)`` searches (``cdf = p.cumsum(); cdf /= cdf[-1]``).
    ``shard_off``: node ranges of the DataLoader workers' shards (graph_dataset.py:23-30,63-76) --
    a worker normalises the weights over ITS graphs, so every range gets its own cdf."""
    w = np.diff(row_ptr).astype(np.float64) ** 0.75
    bounds = [0, len(w)] if shard_off is None or len(shard_off) <= 2 else [int(x) for x in shard_off]
    cdf = np.empty(len(w), dtype=np.float64)
    for a, b in zip(bounds[:-1], bounds[1:]):
        tot = w[a:b].sum()
        if not (np.isfinite(tot) and tot > 0):          # 0/0 would give a NaN cdf and every seed the shard's last node
            raise ValueError(f"seed cdf: the nodes [{a}, {b}) of a worker shard have no edges (total deg^0.75 weight {tot})")
        p = w[a:b] / tot
        c = np.cumsum(p)
        cdf[a:b] = c / c[-1]
    return cdf


def max_nodes_per_seed_table(max_degree: int, rw_hops: int, restart_prob: float) -> np.ndarray:
    """max_nodes_per_seed of graph_dataset.py:113-124 for every in-degree 0..max_degree."""
    # (the reference's order of operations, so that the rounding at x.5 cannot differ: pinned by the reference-executed
    #  tests/golden/getitem_calls_reference.json)
    return np.array([max(rw_hops, int((d ** 0.75) * math.e / (math.e - 1) / restart_prob + 0.5)) for d in range(max_degree + 1)],
                    dtype=np.int32)


def max_nodes_out_degree_table(max_degree: int, rw_hops: int, restart_prob: float, multiplicity: int = 1) -> np.ndarray:
    """max_nodes_per_seed of the GraphDataset family (graph_dataset.py:244-255): the out-degree enters WITHOUT the
    0.75 power; ``multiplicity`` = copies of every edge in the DGL graph the reference walks on."""
    # (the reference's order of operations; pinned by tests/golden/getitem_calls_reference.json)
    return np.array([max(rw_hops, int(d * multiplicity * math.e / (math.e - 1) / restart_prob + 0.5)) for d in range(max_degree + 1)],
                    dtype=np.int32)


HUB_TABLE_DEGREE = 512      # = the sampler's default hub_degree (csrc/sampler.hip kHubDegreeDefault)


def hub_tables(row_ptr: np.ndarray, col_idx: np.ndarray, degree: int = HUB_TABLE_DEGREE, max_bytes: int = 1 << 30):
    """Adjacency among the rows of at least ``degree`` entries (gcc_graph.hub_index / hub_adj): -> (hub_index int32[V],
    hub_adj uint32[H, words]) or None when there are no such rows or the bitmap would exceed ``max_bytes``.  One pass over
    the hub rows' entries (1.6 M on the 1M-node graph, 49 M on the 10M-node one: 1286 / 29,784 hubs, 0.2 / 111 MB)."""
    deg = np.diff(row_ptr)
    hubs = np.flatnonzero(deg >= degree)
    H = int(len(hubs))
    words = (H + 31) // 32
    if H == 0 or H * words * 4 > max_bytes:
        return None
    index = np.full(len(deg), -1, dtype=np.int32)
    index[hubs] = np.arange(H, dtype=np.int32)
    adj = np.zeros((H, words), dtype=np.uint32)
    # entries of the hub rows, row by row in slabs (bounded temporaries)
    starts, lens = row_ptr[hubs].astype(np.int64), deg[hubs].astype(np.int64)
    at = 0
    while at < H:
        end = at
        tot = 0
        while end < H and (tot == 0 or tot + lens[end] <= (1 << 24)):
            tot += int(lens[end])
            end += 1
        rows = np.repeat(np.arange(at, end, dtype=np.int64), lens[at:end])
        offs = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(lens[at:end]) - lens[at:end], lens[at:end])
        cols = index[col_idx[np.repeat(starts[at:end], lens[at:end]) + offs]]
        keep = cols >= 0
        r, c = rows[keep], cols[keep].astype(np.int64)
        np.bitwise_or.at(adj, (r, c >> 5), (np.uint32(1) << (c & 31).astype(np.uint32)))
        at = end
    return index, adj


def restart_threshold(restart_prob: float) -> int:
    """restart <=> 32-bit draw < floor(restart_prob * 2^32)."""
    return min(int(restart_prob * 4294967296.0), 0xFFFFFFFF)


def _max_copies(row_ptr: np.ndarray, col_idx: np.ndarray) -> int:
    """the longest run of equal, adjacent entries within a row (1 on a simple graph)"""
    if len(col_idx) <= 1:
        return 1
    new_run = np.ones(len(col_idx), dtype=bool)
    new_run[1:] = col_idx[1:] != col_idx[:-1]
    starts = row_ptr[:-1]
    new_run[starts[starts < len(col_idx)]] = True      # (an unchecked parent may end in empty rows)
    return int(np.diff(np.append(np.flatnonzero(new_run), len(col_idx))).max())


class DeviceGraph:
    """int32 CSR + seed cdf + max_nodes table on one GPU."""

    def __init__(self, row_ptr: np.ndarray, col_idx: np.ndarray, rw_hops: int = 256,
                 restart_prob: float = 0.8, device="cuda", validate: bool = True, ltab: np.ndarray = None,
                 shard_off=None, trusted: bool = False, hub_table: bool = True, multigraph: bool = False, tables: str = "host"):
        """``validate``: check the input contract (x2dgl.py:39-62) on the host before the upload; ``"device"``: upload first and
        check there (gcc_graph_check: the same violations, the same messages, no SciPy matrices).  ``trusted``: the caller
        vouches for the contract without the check (graphs of gcc_amd.graphgen, whose generator builds to it).  With
        neither, the graph carries no GCC_GRAPH_CONTRACT_CHECKED bit and the induction scans every member row (the hub-row
        short cut of gcc_sample_params.hub_degree is exact on a symmetric, sorted, duplicate- and loop-free parent only).
        ``multigraph``: the parent may hold parallel edges as repeated, adjacent entries of its sorted rows (DGL's
        representation; ``ingest.multigraph_csr``).  It is validated against ``check_multigraph_contract`` and, checked or
        trusted, never carries GCC_GRAPH_CONTRACT_CHECKED and gets no hub tables: a uniform draw over a row's entries is
        the walk on the multigraph and the row-by-row induction emits every copy, but the short cut would not.
        ``tables``: ``"host"`` builds the seed cdf, the hub tables and the degree summary here before the upload;
        ``"device"`` uploads the two arrays as ever and builds them there (gcc_graph_tables: the same integers, a cdf with the
        same properties but not NumPy's bits)."""
        import torch

        if tables not in ("host", "device"):
            raise ValueError(f"tables {tables!r}: \"host\" or \"device\"")
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        col_idx = np.ascontiguousarray(col_idx, dtype=np.int32)
        on_device = isinstance(validate, str)
        if on_device and validate != "device":
            raise ValueError(f"validate {validate!r}: True (the host check), False or \"device\"")
        if validate and not on_device:
            (check_multigraph_contract if multigraph else check_contract)(row_ptr, col_idx)
        self.multigraph = bool(multigraph)
        self.contract_checked = bool(validate or trusted) and not self.multigraph
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceGraph lives in HBM; device must be a HIP/CUDA device")
        if tables == "device":
            self._from_tensors(torch.from_numpy(row_ptr).to(self.device), torch.from_numpy(col_idx).to(self.device), rw_hops, restart_prob,
                               device_check=on_device, vouched=bool(validate or trusted), shard_off=shard_off, hub_table=hub_table,
                               multigraph=multigraph, ltab=ltab, max_copies=_max_copies(row_ptr, col_idx) if multigraph else 1)
            return
        self.num_nodes = int(row_ptr.shape[0] - 1)
        self.num_edges = int(col_idx.shape[0])
        self.rw_hops = int(rw_hops)
        self.restart_prob = float(restart_prob)
        self.restart_u32 = restart_threshold(restart_prob)
        deg = np.diff(row_ptr)
        self.max_degree = int(deg.max())
        d64 = deg.astype(np.float64)
        self.sb_degree = float((d64 * d64).sum() / d64.sum())   # size-biased mean degree: what a random-walk visit sees
        # most parallel edges between one pair: an induced row of a multigraph can hold up to (n - 1) x this many entries
        # (DeviceRWRSampler sizes its edge capacity with it; 1 on a simple parent)
        self.max_copies = _max_copies(row_ptr, col_idx) if self.multigraph else 1
        if ltab is None:
            ltab = max_nodes_per_seed_table(self.max_degree, rw_hops, restart_prob)
        ltab = np.ascontiguousarray(ltab, dtype=np.int32)
        assert ltab.shape[0] == self.max_degree + 1
        self.lmax = int(ltab.max())
        self.row_ptr = torch.from_numpy(row_ptr).to(self.device)
        self.col_idx = torch.from_numpy(col_idx).to(self.device)
        if on_device:                           # the same contract, checked where the graph now lives (gcc_graph_check)
            from .graph_build import GraphBuildEngine

            GraphBuildEngine(device=self.device).validate(self.row_ptr, self.col_idx, multigraph=self.multigraph)
        # worker shards (LoadBalanceGraphDataset): node ranges whose seeds are drawn separately, batch by batch
        self.num_shards = 0
        self.shard_off = None
        if shard_off is not None and len(shard_off) > 2:
            so = np.ascontiguousarray(shard_off, dtype=np.int64)
            if so[0] != 0 or so[-1] != self.num_nodes or np.any(np.diff(so) <= 0):
                raise ValueError("shard_off must be increasing node offsets from 0 to num_nodes (no empty shard)")
            self.num_shards = len(so) - 1
            self.shard_off = torch.from_numpy(so).to(self.device)
        self.seed_cdf = torch.from_numpy(seed_cdf_table(row_ptr, shard_off if self.num_shards else None)).to(self.device)
        self.ltab = torch.from_numpy(ltab).to(self.device)
        # hub-hub adjacency (one bit probe per pair of unscanned hub rows instead of a search): only with a checked contract
        # -- the hub-row short cut is off without it anyway
        self.hub_index = self.hub_adj = None
        self.num_hubs = self.hub_words = 0
        tabs = hub_tables(row_ptr, col_idx) if (self.contract_checked and hub_table) else None
        if tabs is not None:
            self.hub_index = torch.from_numpy(tabs[0]).to(self.device)
            self.hub_adj = torch.from_numpy(tabs[1].view(np.int32)).to(self.device)
            self.num_hubs, self.hub_words = int(tabs[1].shape[0]), int(tabs[1].shape[1])
        self._fill_struct()

    def _fill_struct(self):
        self.c = _cabi.GccGraph(
            hub_index=self.hub_index.data_ptr() if self.hub_index is not None else None,
            hub_adj=self.hub_adj.data_ptr() if self.hub_adj is not None else None,
            num_hubs=self.num_hubs, hub_words=self.hub_words, hub_table_degree=HUB_TABLE_DEGREE if self.num_hubs else 0,
            row_ptr=self.row_ptr.data_ptr(), col_idx=self.col_idx.data_ptr(),
            seed_cdf=self.seed_cdf.data_ptr(), ltab=self.ltab.data_ptr(),
            num_nodes=self.num_nodes, num_edges=self.num_edges,
            ltab_len=int(self.ltab.shape[0]), lmax=self.lmax,
            shard_off=self.shard_off.data_ptr() if self.shard_off is not None else None, num_shards=self.num_shards,
            flags=_cabi.GRAPH_CONTRACT_CHECKED if self.contract_checked else 0)

    @classmethod
    def from_device(cls, row_ptr, col_idx, rw_hops: int = 256, restart_prob: float = 0.8, validate="device", trusted: bool = False,
                    shard_off=None, hub_table: bool = True, multigraph: bool = False, ltab: np.ndarray = None):
        """A DeviceGraph of a CSR that is already in HBM (int32 device tensors, e.g. ``GraphBuildEngine.build``'s): nothing is
        downloaded.  ``validate="device"`` runs gcc_graph_check and raises ``check_contract``'s messages, ``False`` skips it
        (``trusted`` then vouches for the contract as in ``__init__``).  The degree summary, the seed cdf and the hub tables are
        built by gcc_graph_tables; the host reads one status word (when checking) and the summary.  A multigraph needs the
        check: ``max_copies`` comes from its maxima."""
        import torch

        if validate not in ("device", False):
            raise ValueError(f"validate {validate!r}: \"device\" or False (the arrays are not on the host)")
        for name, t in (("row_ptr", row_ptr), ("col_idx", col_idx)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1:
                raise TypeError(f"{name} must be a one-dimensional int32 device tensor")
        if multigraph and not validate:
            raise ValueError("a multigraph from device tensors needs validate=\"device\": max_copies comes from the check's maxima")
        self = cls.__new__(cls)
        self._from_tensors(row_ptr.contiguous(), col_idx.contiguous(), rw_hops, restart_prob, device_check=bool(validate),
                           vouched=bool(trusted), shard_off=shard_off, hub_table=hub_table, multigraph=multigraph, ltab=ltab)
        return self

    def _from_tensors(self, row_ptr, col_idx, rw_hops, restart_prob, device_check, vouched, shard_off, hub_table, multigraph, ltab,
                      max_copies=1):
        """what ``__init__`` fills, from the two arrays where they lie (``tables="device"`` and ``from_device``)"""
        import torch

        from .graph_build import GraphBuildEngine, contract_error
        from .graph_tables import GraphTablesEngine

        self.multigraph = bool(multigraph)
        self.contract_checked = bool(device_check or vouched) and not self.multigraph
        self.device = row_ptr.device
        if self.device.type != "cuda":
            raise RuntimeError("DeviceGraph lives in HBM; device must be a HIP/CUDA device")
        self.num_nodes = int(row_ptr.shape[0] - 1)
        self.num_edges = int(col_idx.shape[0])
        self.rw_hops = int(rw_hops)
        self.restart_prob = float(restart_prob)
        self.restart_u32 = restart_threshold(restart_prob)
        self.row_ptr, self.col_idx = row_ptr, col_idx
        self.max_copies = int(max_copies)
        if device_check:
            res = GraphBuildEngine(device=self.device).check(row_ptr, col_idx, multigraph=self.multigraph)
            text = contract_error(int(res["status"].cpu()[0]), self.multigraph)
            if text:
                raise ValueError(text)
            if self.multigraph:
                self.max_copies = max(int(res["maxima"].cpu()[1]), 1)
        self.num_shards = 0
        self.shard_off = None
        so = None
        if shard_off is not None and len(shard_off) > 2:
            so = np.ascontiguousarray(shard_off, dtype=np.int64)
            if so[0] != 0 or so[-1] != self.num_nodes or np.any(np.diff(so) <= 0):
                raise ValueError("shard_off must be increasing node offsets from 0 to num_nodes (no empty shard)")
            self.num_shards = len(so) - 1
            self.shard_off = torch.from_numpy(so).to(self.device)
        t = GraphTablesEngine(device=self.device).tables(row_ptr, col_idx, so, hub_degree=HUB_TABLE_DEGREE,
                                                         hub_table=self.contract_checked and hub_table)
        self.max_degree = int(t["max_degree"])
        self.sb_degree = float(t["sb_degree"])
        if ltab is None:
            ltab = max_nodes_per_seed_table(self.max_degree, rw_hops, restart_prob)
        ltab = np.ascontiguousarray(ltab, dtype=np.int32)
        assert ltab.shape[0] == self.max_degree + 1
        self.lmax = int(ltab.max())
        self.ltab = torch.from_numpy(ltab).to(self.device)
        self.seed_cdf = t["seed_cdf"]
        self.hub_index, self.hub_adj = t["hub_index"], t["hub_adj"]
        self.num_hubs = self.hub_words = 0
        if self.hub_adj is not None:
            self.num_hubs, self.hub_words = int(self.hub_adj.shape[0]), int(self.hub_adj.shape[1])
        self._fill_struct()

    def byref(self):
        return ctypes.byref(self.c)

    def hbm_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.row_ptr, self.col_idx, self.seed_cdf, self.ltab, self.hub_index, self.hub_adj)
                   if t is not None)
