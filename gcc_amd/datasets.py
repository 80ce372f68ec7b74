"""The GraphDataset family used by the reference's ``generate.py`` (gcc/datasets/graph_dataset.py:180-340), on the
device sampler: one item per NODE of the graph, in node order, both views from the same seed
(``step_dist = [1, 0, 0]``), ``max_nodes_per_seed`` from the out-degree without the 0.75 power (:244-255).

Yields already-batched ``(graph_q, graph_k)`` pairs like ``gcc_amd.sampler.LoadBalanceGraphDataset``; the last batch
is padded with node 0 and reports ``valid`` rows.

``GraphClassificationDataset`` (:306-330): one item per GRAPH of a list of small graphs, ``entire_graph=True``: the
"subgraph" is the whole graph in its own node order, the seed flag marks ``out_degrees().argmax()``
(data_util.py:228-237) and both views are identical (the random walk's result is discarded), so batches are
assembled without the sampler: on the device by gcc_pack_graphs from a resident corpus (``batcher="device"``, what
``"auto"`` picks on a GPU), or by the host loop (``batcher="host"``, the yardstick the device batcher is tested against)."""
from __future__ import annotations

import ctypes
import functools

import numpy as np

from .graph import max_nodes_out_degree_table


def resolve_batcher(batcher, device):
    """``"auto"`` -> ``"device"`` on a GPU and ``"host"`` otherwise; ``"device"`` off the GPU is refused by name"""
    import torch

    if batcher not in ("auto", "host", "device"):
        raise ValueError(f'batcher must be "auto", "host" or "device" (got {batcher!r})')
    on_gpu = torch.device(device).type == "cuda"
    if batcher == "device" and not on_gpu:
        raise ValueError(f'batcher="device" needs a GPU device (got {device!r}): gcc_pack_graphs has no CPU path, '
                         'use batcher="host"')
    return "device" if batcher == "device" or (batcher == "auto" and on_gpu) else "host"


class DeviceGraphCorpus:
    """Every graph of a whole-graph dataset, concatenated and resident on the device (gcc_graph_corpus), plus a ring of
    ``num_buffers`` output buffer sets; :meth:`pack` issues one gcc_pack_graphs call into the next set.  A set is rewritten
    ``num_buffers`` calls later, so a consumer that keeps ``k`` batches in flight needs ``k + 1`` sets (LabeledProducer:
    ``depth + 2``).  ``lib`` / ``ptr`` are injectable for the emulator tests only."""

    _BITS = ((1, "node capacity"), (2, "edge capacity"), (4, "graph index out of range"))

    def __init__(self, graphs, batch_size, labels=None, pos_dim=0, expand=1, device="cuda", num_buffers=3, node_cap=None,
                 edge_cap=None, placeholder=True, lib=None, ptr=None):
        import torch

        from . import _cabi

        self.lib = lib if lib is not None else _cabi.load()
        self.ptr = ptr if ptr is not None else _cabi.dev_ptr
        self.device, self.batch_size, self.pos_dim, self.expand = device, int(batch_size), int(pos_dim), max(int(expand), 1)
        if not 1 <= self.batch_size <= _cabi.PACK_GRAPHS_MAX_BATCH:
            raise ValueError(f"the device batcher packs 1..{_cabi.PACK_GRAPHS_MAX_BATCH} graphs per batch "
                             f"(GCC_PACK_GRAPHS_MAX_BATCH), got batch_size {self.batch_size}; use batcher=\"host\"")
        if self.pos_dim and (self.pos_dim < 2 or self.pos_dim % 2):
            raise ValueError(f"positional rows must have an even size of at least 2 (got {self.pos_dim})")
        self.sizes = np.array([len(rp) - 1 for rp, _ in graphs], dtype=np.int64)
        self.entries = np.array([len(ci) for _, ci in graphs], dtype=np.int64)       # live col_idx length of a batch: a host sum
        self.first = np.concatenate([[0], np.cumsum(self.sizes)])
        efirst = np.concatenate([[0], np.cumsum(self.entries)])
        if self.first[-1] >= 2 ** 31 - 1 or efirst[-1] >= 2 ** 31 - 1:
            raise ValueError("the corpus does not fit int32 offsets")
        G = len(graphs)
        row_ptr = np.zeros(int(self.first[-1]) + 1, dtype=np.int32)
        seed_local = np.zeros(G, dtype=np.int32)
        for g, (rp, _) in enumerate(graphs):
            rp = np.asarray(rp, dtype=np.int64)
            row_ptr[self.first[g] + 1: self.first[g + 1] + 1] = rp[1:] + efirst[g]
            if len(rp) > 1:
                seed_local[g] = int(np.argmax(np.diff(rp)))             # out_degrees().argmax(), first maximum (_convert_idx)
        col_idx = (np.concatenate([np.asarray(ci, dtype=np.int32) for _, ci in graphs]) if G and efirst[-1]
                   else np.zeros(1, dtype=np.int32))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)          # noqa: E731
        self.node_first = up(self.first.astype(np.int32))
        self.row_ptr, self.col_idx, self.seed_local = up(row_ptr), up(col_idx), up(seed_local)
        self.labels = up(np.asarray(labels).astype(np.int32)) if labels is not None else None
        self.pos = None
        self.c = _cabi.GccGraphCorpus(num_graphs=G, pos_dim=self.pos_dim, node_first=self.ptr(self.node_first),
                                      row_ptr=self.ptr(self.row_ptr), col_idx=self.ptr(self.col_idx),
                                      seed_local=self.ptr(self.seed_local),
                                      labels=self.ptr(self.labels) if self.labels is not None else None, pos=None)
        B = self.batch_size
        largest, most = int(self.sizes.max()) if G else 0, int(self.entries.max()) if G else 0
        self.node_cap = int(node_cap) if node_cap is not None else B * (largest + 1)   # (the eigensolver's convention)
        self.edge_cap = int(edge_cap) if edge_cap is not None else max(B * most * self.expand, 1)
        i32 = dict(dtype=torch.int32, device=device)
        self.status = torch.zeros(1, **i32)
        self.parent_nid = torch.zeros(self.node_cap, **i32)              # never written: the zero buffer of the host batches
        # col_idx of an edge-free batch: the host's one-element placeholder, repeated like every entry
        self._placeholder = torch.zeros(self.expand, **i32) if placeholder else None
        self._ring = []
        for _ in range(max(int(num_buffers), 1)):
            slot = dict(node_off=torch.zeros(B + 1, **i32), edge_off=torch.zeros(B + 1, **i32),
                        graph_id=torch.zeros(self.node_cap, **i32), row_ptr=torch.zeros(self.node_cap + 1, **i32),
                        col_idx=torch.zeros(self.edge_cap, **i32), seed_local=torch.zeros(B, **i32),
                        labels=torch.full((B,), -1, **i32))
            if self.pos_dim:
                slot["pos"] = torch.zeros(self.node_cap, self.pos_dim, dtype=torch.float32, device=device)
            self._ring.append(slot)
        self._next = 0

    @classmethod
    def from_device(cls, corpus, batch_size, with_labels=True, pos_dim=0, expand=1, device=None, num_buffers=3, node_cap=None,
                    edge_cap=None, placeholder=True, lib=None, ptr=None):
        """The corpus that is already resident (``TUIngestEngine.read_tudataset(...)["corpus"]``: node_first, row_ptr, col_idx,
        seed_local, labels as int32 device tensors; sizes, entries as host int64): the same members as ``__init__`` fills, with
        no per-graph loop and no upload.  ``with_labels=False``: the unlabelled corpus (``labels=None`` of ``__init__``)."""
        import torch

        from . import _cabi

        self = cls.__new__(cls)
        self.lib = lib if lib is not None else _cabi.load()
        self.ptr = ptr if ptr is not None else _cabi.dev_ptr
        self.device = device if device is not None else corpus["row_ptr"].device
        self.batch_size, self.pos_dim, self.expand = int(batch_size), int(pos_dim), max(int(expand), 1)
        if not 1 <= self.batch_size <= _cabi.PACK_GRAPHS_MAX_BATCH:
            raise ValueError(f"the device batcher packs 1..{_cabi.PACK_GRAPHS_MAX_BATCH} graphs per batch "
                             f"(GCC_PACK_GRAPHS_MAX_BATCH), got batch_size {self.batch_size}; use batcher=\"host\"")
        if self.pos_dim and (self.pos_dim < 2 or self.pos_dim % 2):
            raise ValueError(f"positional rows must have an even size of at least 2 (got {self.pos_dim})")
        self.sizes = np.asarray(corpus["sizes"], dtype=np.int64)
        self.entries = np.asarray(corpus["entries"], dtype=np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.sizes)])
        G = len(self.sizes)
        for name, words in (("node_first", G + 1), ("row_ptr", int(self.first[-1]) + 1), ("col_idx", max(int(self.entries.sum()), 1)),
                            ("seed_local", G), ("labels", G)):
            t = corpus[name]
            if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != words or not t.is_contiguous():
                raise ValueError(f"corpus[{name!r}] must be a contiguous int32 tensor of {words} words")
        self.node_first, self.row_ptr, self.col_idx = corpus["node_first"], corpus["row_ptr"], corpus["col_idx"]
        self.seed_local = corpus["seed_local"]
        self.labels = corpus["labels"] if with_labels else None
        self.pos = None
        self.c = _cabi.GccGraphCorpus(num_graphs=G, pos_dim=self.pos_dim, node_first=self.ptr(self.node_first),
                                      row_ptr=self.ptr(self.row_ptr), col_idx=self.ptr(self.col_idx),
                                      seed_local=self.ptr(self.seed_local),
                                      labels=self.ptr(self.labels) if self.labels is not None else None, pos=None)
        B = self.batch_size
        largest, most = int(self.sizes.max()) if G else 0, int(self.entries.max()) if G else 0
        self.node_cap = int(node_cap) if node_cap is not None else B * (largest + 1)
        self.edge_cap = int(edge_cap) if edge_cap is not None else max(B * most * self.expand, 1)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.status = torch.zeros(1, **i32)
        self.parent_nid = torch.zeros(self.node_cap, **i32)
        self._placeholder = torch.zeros(self.expand, **i32) if placeholder else None
        self._ring = []
        for _ in range(max(int(num_buffers), 1)):
            slot = dict(node_off=torch.zeros(B + 1, **i32), edge_off=torch.zeros(B + 1, **i32),
                        graph_id=torch.zeros(self.node_cap, **i32), row_ptr=torch.zeros(self.node_cap + 1, **i32),
                        col_idx=torch.zeros(self.edge_cap, **i32), seed_local=torch.zeros(B, **i32),
                        labels=torch.full((B,), -1, **i32))
            if self.pos_dim:
                slot["pos"] = torch.zeros(self.node_cap, self.pos_dim, dtype=torch.float32, device=self.device)
            self._ring.append(slot)
        self._next = 0
        return self

    def set_pos(self, pos):
        """the table of every graph's positional rows [sum of nodes, pos_dim] (float32, on the device), once it exists"""
        import torch

        if pos is self.pos:
            return
        if pos.dtype != torch.float32 or tuple(pos.shape) != (int(self.first[-1]), self.pos_dim) or not pos.is_contiguous():
            raise ValueError(f"the positional table must be contiguous float32 [{int(self.first[-1])}, {self.pos_dim}]")
        self.pos = pos
        self.c.pos = self.ptr(pos)

    def index_tensor(self, idx):
        """graph indices -> int32 device tensor padded with -1 to a multiple of the batch size (one upload)"""
        import torch

        idx = np.asarray(idx, dtype=np.int64)
        B = self.batch_size
        padded = np.full(max((len(idx) + B - 1) // B, 1) * B, -1, dtype=np.int32)
        padded[: len(idx)] = idx
        return torch.from_numpy(padded).to(self.device)

    def pack(self, idx_dev, live_entries, expand=None, with_pos=True):
        """One gcc_pack_graphs call: ``idx_dev`` int32 [batch_size] on the device (-1 = padding), ``live_entries`` the sum of
        the selected graphs' entry counts (known on the host: ``entries[idx].sum()``).  -> (BatchedCSR, labels int32 [B])"""
        from . import _cabi
        from .sampler import BatchedCSR

        B = self.batch_size
        expand = self.expand if expand is None else int(expand)
        assert idx_dev.numel() == B and 1 <= expand <= self.expand
        slot = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        e = int(live_entries) * expand
        col = slot["col_idx"][:e] if e or self._placeholder is None else self._placeholder[:expand]
        g = BatchedCSR(B, slot["node_off"], slot["edge_off"], self.parent_nid, slot["graph_id"], slot["row_ptr"], col)
        out = _cabi.GccBatchOut(node_off=self.ptr(slot["node_off"]), edge_off=self.ptr(slot["edge_off"]),
                                parent_nid=self.ptr(self.parent_nid), graph_id=self.ptr(slot["graph_id"]),
                                row_ptr=self.ptr(slot["row_ptr"]), col_idx=self.ptr(slot["col_idx"]),
                                node_cap=self.node_cap, edge_cap=self.edge_cap)
        pos = slot["pos"] if with_pos and self.pos is not None else None
        _cabi.call(self.lib, "gcc_pack_graphs", ctypes.byref(self.c), self.ptr(idx_dev), B, ctypes.byref(out),
                   self.ptr(pos) if pos is not None else None, self.ptr(slot["seed_local"]), self.ptr(slot["labels"]), expand,
                   self.ptr(self.status), _cabi.raw_stream(self.device))
        g.seed_local = slot["seed_local"]
        if pos is not None:
            g.pos_undirected = pos
        return g, slot["labels"]

    def check_status(self) -> None:
        """Synchronising check of the batcher's status word (raises on any bit, never truncates silently)."""
        s = int(self.status.item())
        if s:
            raise RuntimeError("gcc_pack_graphs: " + ", ".join(n for b, n in self._BITS if s & b) +
                               " -- the batch was cut at a graph boundary")


class NodeClassificationDataset:
    def __init__(self, dataset=None, rw_hops=64, subgraph_size=64, restart_prob=0.8, positional_embedding_size=32,
                 step_dist=(1.0, 0.0, 0.0), graph=None, edge_multiplicity=2, batch_size=256, run_seed=0,
                 device="cuda", sample_fn=None, multigraph=False):
        """``graph`` = (row_ptr, col_idx) of the SIMPLE symmetric graph; ``edge_multiplicity`` = copies of every edge in
        the reference's DGL graph (gcc_amd.ingest.read_edgelist reports it).  ``sample_fn(first_id, seeds) -> (q, k)``
        is injectable for the emulator tests.
        ``multigraph``: ``graph`` holds parallel edges as repeated entries of its sorted rows (gcc_amd.ingest.multigraph_csr,
        read_ss_graph(csr=True)) and ``edge_multiplicity`` is only the uniform factor on top (the 2 of the reference's
        double insertion).  The row lengths are then the multigraph's degrees, so the out-degree rule below
        (graph_dataset.py:244-255) needs nothing else; the flag goes to DeviceGraph, which validates the multigraph contract
        and keeps the induction scanning every row."""
        if list(step_dist) != [1.0, 0.0, 0.0]:
            raise NotImplementedError("step_dist other than [1, 0, 0] (generate.py and train.py never pass one)")
        assert positional_embedding_size > 1                       # graph_dataset.py:290
        if graph is None:
            raise ValueError("pass graph=(row_ptr, col_idx); named datasets need their files (gcc_amd.ingest)")
        self.dataset = dataset
        self.rw_hops, self.subgraph_size, self.restart_prob = rw_hops, subgraph_size, restart_prob
        self.positional_embedding_size = positional_embedding_size
        self.step_dist = list(step_dist)
        self.edge_multiplicity = int(edge_multiplicity)
        self.batch_size = int(batch_size)
        self.multigraph = bool(multigraph)
        row_ptr, col_idx = graph
        self.length = int(len(row_ptr) - 1)                        # one item per node, :293
        self.total = self.length
        self.ltab = max_nodes_out_degree_table(int(np.diff(row_ptr).max()), rw_hops, restart_prob, self.edge_multiplicity)
        self._sample = sample_fn
        if sample_fn is None:
            from .graph import DeviceGraph
            from .sampler import DeviceRWRSampler

            self.graph = DeviceGraph(row_ptr, col_idx, rw_hops=rw_hops, restart_prob=restart_prob, device=device,
                                     ltab=self.ltab, multigraph=self.multigraph)
            self.sampler = DeviceRWRSampler(self.graph, self.batch_size, run_seed=run_seed)
            self._sample = self._device_sample

    def _device_sample(self, first_id, seeds):
        import torch

        return self.sampler.sample(first_id, seeds=torch.from_numpy(seeds).to(self.graph.device))

    def __len__(self):
        return self.length

    def num_batches(self):
        return (self.length + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        B = self.batch_size
        for i in range(self.num_batches()):
            lo = i * B
            valid = min(B, self.length - lo)
            seeds = np.zeros(B, dtype=np.int32)
            seeds[:valid] = np.arange(lo, lo + valid, dtype=np.int32)
            q, k = self._sample(lo, seeds)
            for g in (q, k):
                g.edge_multiplicity = self.edge_multiplicity
                g.valid = valid
            yield q, k


class GraphClassificationDataset:
    def __init__(self, dataset=None, rw_hops=64, subgraph_size=64, restart_prob=0.8, positional_embedding_size=32,
                 step_dist=(1.0, 0.0, 0.0), graphs=None, edge_multiplicity=1, batch_size=256, device="cuda", batcher="auto",
                 num_buffers=2, corpus=None):
        """``graphs``: list of (row_ptr, col_idx) of simple symmetric graphs (what TUDataset holds for
        imdb-binary / imdb-multi / rdt-b / rdt-5k / collab); the dataset files themselves are not bundled.
        ``batcher``: ``"device"`` (gcc_pack_graphs from a resident corpus into a ring of ``num_buffers`` buffer sets; what
        ``"auto"`` means on a GPU) or ``"host"`` (the NumPy loop below; ``"auto"`` off the GPU).
        ``corpus``: instead of ``graphs``, the tables that are already on the device
        (``TUIngestEngine.read_tudataset(...)["corpus"]``); the batcher is then the device one and the host list does not exist."""
        if list(step_dist) != [1.0, 0.0, 0.0]:
            raise NotImplementedError("step_dist other than [1, 0, 0]")
        assert positional_embedding_size > 1
        if graphs is None and corpus is None:
            raise ValueError("pass graphs=[(row_ptr, col_idx), ...] or corpus= (the resident tables of TUIngestEngine)")
        if graphs is not None and corpus is not None:
            raise ValueError("pass graphs= or corpus=, not both")
        if corpus is not None and batcher == "host":
            raise ValueError('batcher="host" needs graphs=: a resident corpus= holds no host list to batch from')
        self.dataset, self.entire_graph = dataset, True               # graph_dataset.py:320
        self.rw_hops, self.subgraph_size, self.restart_prob = rw_hops, subgraph_size, restart_prob
        self.positional_embedding_size = positional_embedding_size
        self.corpus_tables = corpus
        self.graphs = ([(np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)) for rp, ci in graphs]
                       if corpus is None else None)
        self.length = self.total = len(self.graphs) if corpus is None else len(corpus["sizes"])
        self.edge_multiplicity = int(edge_multiplicity)
        self.batch_size = int(batch_size)
        self.device = device
        # capacity convention of the pipeline (as DeviceRWRSampler: B * (largest subgraph + 1)): the eigensolver sizes its
        # per-subgraph workspace as node_cap / batch_size
        largest = max(len(rp) - 1 for rp, _ in self.graphs) if corpus is None else int(np.max(corpus["sizes"]))
        self.node_cap = self.batch_size * (largest + 1)
        self.batcher = resolve_batcher(batcher if corpus is None else "device", device)
        self.num_buffers = int(num_buffers)
        self._corpus = None                                           # DeviceGraphCorpus, uploaded on first use

    def __len__(self):
        return self.length

    def _device_corpus(self):
        if self._corpus is None and self.corpus_tables is not None:
            self._corpus = DeviceGraphCorpus.from_device(self.corpus_tables, self.batch_size, with_labels=False, device=self.device,
                                                         num_buffers=self.num_buffers, node_cap=self.node_cap, placeholder=False)
        if self._corpus is None:
            self._corpus = DeviceGraphCorpus(self.graphs, self.batch_size, device=self.device, num_buffers=self.num_buffers,
                                             node_cap=self.node_cap, placeholder=False)
        return self._corpus

    def _need_graphs(self, what):
        if self.graphs is None:
            raise RuntimeError(f"{what} needs the host list graphs=; this dataset was built from a resident corpus=")

    def check_status(self):
        if self._corpus is not None:
            self._corpus.check_status()

    def _convert_idx(self, idx):                                      # :326-329
        self._need_graphs("_convert_idx")
        rp, _ = self.graphs[idx]
        return idx, int(np.argmax(np.diff(rp)))

    def _batch_of(self, idx):
        """The host batcher: the graphs ``idx`` (at most batch_size indices, in any order) as one batch, padded with empty graphs.
        row_ptr always starts with its [0] row, and a batch without entries gets a one-element col_idx (a null address is
        refused further down)."""
        import torch

        from .sampler import BatchedCSR

        self._need_graphs("_batch_of")
        B = self.batch_size
        node_off, edge_off, rows, cols, seeds = [0], [0], [np.zeros(1, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], []
        for i in idx:
            rp, ci = self.graphs[i]
            o = node_off[-1]
            rows.append(rp[1:] + edge_off[-1])
            cols.append(ci + o)
            seeds.append(self._convert_idx(i)[1])
            node_off.append(o + len(rp) - 1)
            edge_off.append(edge_off[-1] + len(ci))
        for _ in range(len(idx), B):
            node_off.append(node_off[-1])
            edge_off.append(edge_off[-1])
            seeds.append(0)
        n = node_off[-1]
        i32 = dict(dtype=torch.int32, device=self.device)
        row_ptr = torch.zeros(self.node_cap + 1, **i32)
        row_ptr[: n + 1] = torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(self.device)
        graph_id = torch.zeros(self.node_cap, **i32)
        graph_id[:n] = torch.repeat_interleave(torch.arange(B, dtype=torch.int32), torch.tensor(np.diff(node_off))).to(self.device)
        col = np.concatenate(cols).astype(np.int32)
        g = BatchedCSR(B, torch.tensor(node_off, **i32), torch.tensor(edge_off, **i32), torch.zeros(self.node_cap, **i32),
                       graph_id, row_ptr, torch.from_numpy(col if len(col) else np.zeros(1, np.int32)).to(self.device))
        g.seed_local = torch.tensor(seeds, **i32)
        g.edge_multiplicity = self.edge_multiplicity
        g.valid = len(idx)
        return g

    def __iter__(self):
        if self.batcher == "device":
            yield from self._iter_device()
            return
        for lo in range(0, self.length, self.batch_size):
            g = self._batch_of(range(lo, min(lo + self.batch_size, self.length)))
            yield g, g                                                # graph_q and graph_k are the same whole graph

    def _iter_device(self):
        corpus, B = self._device_corpus(), self.batch_size
        order = corpus.index_tensor(np.arange(self.length))           # one upload; every batch passes a slice of it
        for lo in range(0, self.length, B):
            hi = min(lo + B, self.length)
            g, _ = corpus.pack(order[lo:lo + B], corpus.entries[lo:hi].sum(), expand=1, with_pos=False)
            g.edge_multiplicity = self.edge_multiplicity              # (kept on the batch, as the host batches do)
            g.valid = hi - lo
            yield g, g


# ------------------------------------------------------------------------------------------------ labelled (--finetune)
def _flatten_tail(g, valid):
    """Rows valid..B-1 of a batch become EMPTY subgraphs (flat node_off / edge_off tail): a partial last batch then gives
    exactly the reference's result for the smaller batch -- no node of a padding row enters the BatchNorm statistics, and the
    head (gcc_cls_head_train) skips rows labelled -1."""
    if valid < g.batch_size:
        g.node_off[valid + 1:] = g.node_off[valid]
        g.edge_off[valid + 1:] = g.edge_off[valid]
    g.valid = valid
    return g


def _expand_multiplicity(g):
    """Training on a multigraph parent (every edge ``edge_multiplicity`` times in the reference's DGL graph): the GIN backward
    takes simple CSR only, so every CSR entry is repeated in place of the multiplicity -- row r's entries, each
    ``edge_multiplicity`` times in a row.  The sum aggregation and the in-degrees are then exactly the multigraph's.  Sized by
    the buffers' capacity, so no host read of the live edge count.  (Run after the positional embedding: the normalised
    Laplacian of a uniformly multiplied graph is the simple graph's.)"""
    m = int(g.edge_multiplicity)
    if m > 1:
        g.row_ptr = g.row_ptr * m
        g.edge_off = g.edge_off * m
        g.col_idx = g.col_idx.unsqueeze(1).expand(-1, m).reshape(-1).contiguous()
        g.edge_multiplicity = 1
    return g


class NodeClassificationDatasetLabeled:
    """graph_dataset.py:388-433 on the device sampler: one item per node, ONE RWR view seeded at that node with the constant
    ``max_nodes_per_seed = rw_hops`` (not the out-degree formula of the unlabelled classes), label ``y[idx].argmax()``.
    Only that view is position-embedded.  :meth:`batches` takes the item order (a fold's indices, permuted per epoch by the
    caller) and yields ``(graph_q, labels)`` with ``labels`` int32 [B] on the device, -1 on the padding rows of a partial
    last batch."""

    def __init__(self, dataset=None, rw_hops=64, subgraph_size=64, restart_prob=0.8, positional_embedding_size=32,
                 graph=None, labels=None, edge_multiplicity=2, batch_size=32, run_seed=0, device="cuda", num_buffers=3):
        if graph is None or labels is None:
            raise ValueError("pass graph=(row_ptr, col_idx) and labels (node classification needs --nodelabel)")
        labels = np.asarray(labels)
        if labels.ndim == 2:                                           # one-hot y (ingest.read_edgelist): y.argmax(1)
            labels = labels.argmax(1)
        self.dataset = dataset
        self.rw_hops, self.subgraph_size, self.restart_prob = rw_hops, subgraph_size, restart_prob
        self.positional_embedding_size = positional_embedding_size
        self.edge_multiplicity = int(edge_multiplicity)
        self.batch_size = int(batch_size)
        self.labels = labels.astype(np.int64)
        self.num_classes = int(self.labels.max()) + 1
        row_ptr, col_idx = graph
        self.length = self.total = int(len(row_ptr) - 1)
        assert len(self.labels) == self.length, "one label per node"
        self.ltab = np.full(int(np.diff(row_ptr).max()) + 1, rw_hops, dtype=np.int32)       # graph_dataset.py:417
        self.device = device
        self._sample_id = 0
        from .graph import DeviceGraph
        from .posemb import DevicePosEmb
        from .sampler import DeviceRWRSampler

        self.graph = DeviceGraph(row_ptr, col_idx, rw_hops=rw_hops, restart_prob=restart_prob, device=device, ltab=self.ltab)
        self.sampler = DeviceRWRSampler(self.graph, self.batch_size, run_seed=run_seed, num_buffers=num_buffers)
        self.posemb = DevicePosEmb(self.batch_size, self.sampler.node_cap, positional_embedding_size, device=device,
                                   seed=run_seed, num_buffers=num_buffers)

    def __len__(self):
        return self.length

    def make_batch(self, idx):
        """the batch of items ``idx`` (at most batch_size node ids): sample, pad, embed the q view -> (graph_q, labels)"""
        import torch

        B, valid = self.batch_size, len(idx)
        seeds = np.zeros(B, dtype=np.int32)
        seeds[:valid] = idx
        lab = np.full(B, -1, dtype=np.int32)
        lab[:valid] = self.labels[idx]
        q, _k = self.sampler.sample(self._sample_id, seeds=torch.from_numpy(seeds).to(self.device))
        self._sample_id += B
        q.edge_multiplicity = self.edge_multiplicity
        _flatten_tail(q, valid)
        self.posemb(q)                                                 # the q view only: the k view is never read
        _expand_multiplicity(q)
        return q, torch.from_numpy(lab).to(self.device)

    def batches(self, order):
        order = np.asarray(order, dtype=np.int64)
        for lo in range(0, len(order), self.batch_size):
            yield self.make_batch(order[lo:lo + self.batch_size])

    def check_status(self):
        self.sampler.check_status()
        self.posemb.check_status()


class GraphClassificationDatasetLabeled(GraphClassificationDataset):
    """graph_dataset.py:342-385: one item per graph, the whole graph (``entire_graph=True``), label ``graph_labels[idx]``.
    The reference computes every item once (``self.dict``), so a graph's positional embedding is computed once -- here on the
    first use, in batches over all graphs -- and gathered into each batch afterwards."""

    def __init__(self, dataset=None, rw_hops=64, subgraph_size=64, restart_prob=0.8, positional_embedding_size=32,
                 graphs=None, labels=None, edge_multiplicity=1, batch_size=32, run_seed=0, device="cuda", batcher="auto",
                 num_buffers=3, corpus=None):
        super().__init__(dataset=dataset, rw_hops=rw_hops, subgraph_size=subgraph_size, restart_prob=restart_prob,
                         positional_embedding_size=positional_embedding_size, graphs=graphs,
                         edge_multiplicity=edge_multiplicity, batch_size=batch_size, device=device, batcher=batcher,
                         num_buffers=num_buffers, corpus=corpus)
        if labels is None and corpus is not None:
            labels = corpus["labels"].cpu().numpy()                    # (the corpus' own, re-indexed 0..C-1)
        if labels is None:
            raise ValueError("pass labels (graph_labels of the TU dataset)")
        self.labels = np.asarray(labels).astype(np.int64)
        assert len(self.labels) == self.length, "one label per graph"
        self.num_classes = int(self.labels.max()) + 1
        self.run_seed = run_seed
        self.sizes = (np.array([len(rp) - 1 for rp, _ in self.graphs], dtype=np.int64) if corpus is None
                      else np.asarray(corpus["sizes"], dtype=np.int64))
        self.first = np.concatenate([[0], np.cumsum(self.sizes)])
        self._pos = None                                               # [sum of nodes, P] on the device, every graph once
        self.posemb = None

    def _device_corpus(self):
        if self._corpus is None and self.corpus_tables is not None:
            self._corpus = DeviceGraphCorpus.from_device(self.corpus_tables, self.batch_size, pos_dim=self.positional_embedding_size,
                                                         expand=self.edge_multiplicity, device=self.device,
                                                         num_buffers=self.num_buffers, node_cap=self.node_cap)
        if self._corpus is None:
            self._corpus = DeviceGraphCorpus(self.graphs, self.batch_size, labels=self.labels,
                                             pos_dim=self.positional_embedding_size, expand=self.edge_multiplicity,
                                             device=self.device, num_buffers=self.num_buffers, node_cap=self.node_cap)
        return self._corpus

    def _embed_all(self):
        import torch

        from .posemb import DevicePosEmb

        self.posemb = DevicePosEmb(self.batch_size, self.node_cap, self.positional_embedding_size, device=self.device,
                                   seed=self.run_seed, num_buffers=1)
        if self.batcher == "device":                                   # the same batches, idx = arange, simple CSR
            corpus, B = self._device_corpus(), self.batch_size
            order = corpus.index_tensor(np.arange(self.length))
            table = torch.zeros(int(self.first[-1]), self.positional_embedding_size, dtype=torch.float32, device=self.device)
            for lo in range(0, self.length, B):
                hi = min(lo + B, self.length)
                g, _ = corpus.pack(order[lo:lo + B], corpus.entries[lo:hi].sum(), expand=1, with_pos=False)
                self.posemb(g)
                a, b = int(self.first[lo]), int(self.first[hi])
                table[a:b].copy_(g.pos_undirected[: b - a])
            self._pos = table
            return
        parts = []
        for lo in range(0, self.length, self.batch_size):
            idx = np.arange(lo, min(lo + self.batch_size, self.length))
            g = self._batch_of(idx)
            self.posemb(g)
            parts.append(g.pos_undirected[: int(self.first[idx[-1] + 1] - self.first[idx[0]])].clone())
        self._pos = torch.cat(parts)

    def _device_batch(self, idx_dev, idx, ready=None):
        """the batch of the graphs ``idx`` whose indices are already on the device (``idx_dev``: int32 [B], -1 = padding)"""
        import torch

        if self._pos is None:
            self._embed_all()
        corpus = self._device_corpus()
        corpus.set_pos(self._pos)
        if ready is not None:                                          # the upload may have been issued on another stream
            torch.cuda.current_stream(self.device).wait_event(ready)
        g, lab = corpus.pack(idx_dev, corpus.entries[idx].sum())       # entries repeated edge_multiplicity times in place
        g.edge_multiplicity = 1
        g.valid = len(idx)
        return g, lab

    def batch_calls(self, order):
        """one callable per batch of ``order``; the device batcher uploads the whole order once (padded with -1) and every
        call passes a slice of it, so a batch costs no host-to-device copy"""
        import torch

        order = np.asarray(order, dtype=np.int64)
        chunks = [order[lo:lo + self.batch_size] for lo in range(0, len(order), self.batch_size)]
        if self.batcher != "device":
            return [functools.partial(self.make_batch, c) for c in chunks]
        B = self.batch_size
        order_dev = self._device_corpus().index_tensor(order)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        return [functools.partial(self._device_batch, order_dev[i * B:(i + 1) * B], c, ready) for i, c in enumerate(chunks)]

    def make_batch(self, idx):
        import torch

        if self.batcher == "device":
            idx = np.asarray(idx, dtype=np.int64)
            return self._device_batch(self._device_corpus().index_tensor(idx), idx)
        if self._pos is None:
            self._embed_all()
        idx = np.asarray(idx, dtype=np.int64)
        g = self._batch_of(idx)
        rows = np.concatenate([np.arange(self.first[i], self.first[i + 1]) for i in idx]) if len(idx) else np.zeros(0, np.int64)
        pos = torch.zeros(self.node_cap, self.positional_embedding_size, dtype=torch.float32, device=self.device)
        if len(rows):
            pos[: len(rows)] = self._pos[torch.from_numpy(rows).to(self.device)]
        g.pos_undirected = pos
        _expand_multiplicity(g)
        lab = np.full(self.batch_size, -1, dtype=np.int32)
        lab[: len(idx)] = self.labels[idx]
        return g, torch.from_numpy(lab).to(self.device)

    def batches(self, order):
        if self.batcher == "device":
            for call in self.batch_calls(order):
                yield call()
            return
        order = np.asarray(order, dtype=np.int64)
        for lo in range(0, len(order), self.batch_size):
            yield self.make_batch(order[lo:lo + self.batch_size])

    def check_status(self):
        super().check_status()
        if self.posemb is not None:
            self.posemb.check_status()
