"""The GraphDataset family used by the reference's ``generate.py`` (gcc/datasets/graph_dataset.py:180-340), on the
device sampler: one item per NODE of the graph, in node order, both views from the same seed
(``step_dist = [1, 0, 0]``), ``max_nodes_per_seed`` from the out-degree without the 0.75 power (:244-255).

Yields already-batched ``(graph_q, graph_k)`` pairs like ``gcc_amd.sampler.LoadBalanceGraphDataset``; the last batch
is padded with node 0 and reports ``valid`` rows.

``GraphClassificationDataset`` (:306-330): one item per GRAPH of a list of small graphs, ``entire_graph=True``: the
"subgraph" is the whole graph in its own node order, the seed flag marks ``out_degrees().argmax()``
(data_util.py:228-237) and both views are identical (the random walk's result is discarded), so batches are
assembled without the sampler."""
from __future__ import annotations

import numpy as np

from .graph import max_nodes_out_degree_table


class NodeClassificationDataset:
    def __init__(self, dataset=None, rw_hops=64, subgraph_size=64, restart_prob=0.8, positional_embedding_size=32,
                 step_dist=(1.0, 0.0, 0.0), graph=None, edge_multiplicity=2, batch_size=256, run_seed=0,
                 device="cuda", sample_fn=None):
        """``graph`` = (row_ptr, col_idx) of the SIMPLE symmetric graph; ``edge_multiplicity`` = copies of every edge in
        the reference's DGL graph (gcc_amd.ingest.read_edgelist reports it).  ``sample_fn(first_id, seeds) -> (q, k)``
        is injectable for the emulator tests."""
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
        row_ptr, col_idx = graph
        self.length = int(len(row_ptr) - 1)                        # one item per node, :293
        self.total = self.length
        self.ltab = max_nodes_out_degree_table(int(np.diff(row_ptr).max()), rw_hops, restart_prob, self.edge_multiplicity)
        self._sample = sample_fn
        if sample_fn is None:
            from .graph import DeviceGraph
            from .sampler import DeviceRWRSampler

            self.graph = DeviceGraph(row_ptr, col_idx, rw_hops=rw_hops, restart_prob=restart_prob, device=device,
                                     ltab=self.ltab)
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
                 step_dist=(1.0, 0.0, 0.0), graphs=None, edge_multiplicity=1, batch_size=256, device="cuda"):
        """``graphs``: list of (row_ptr, col_idx) of simple symmetric graphs (what TUDataset holds for
        imdb-binary / imdb-multi / rdt-b / rdt-5k / collab); the dataset files themselves are not bundled."""
        if list(step_dist) != [1.0, 0.0, 0.0]:
            raise NotImplementedError("step_dist other than [1, 0, 0]")
        assert positional_embedding_size > 1
        if graphs is None:
            raise ValueError("pass graphs=[(row_ptr, col_idx), ...]")
        self.dataset, self.entire_graph = dataset, True               # graph_dataset.py:320
        self.rw_hops, self.subgraph_size, self.restart_prob = rw_hops, subgraph_size, restart_prob
        self.positional_embedding_size = positional_embedding_size
        self.graphs = [(np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)) for rp, ci in graphs]
        self.length = self.total = len(self.graphs)
        self.edge_multiplicity = int(edge_multiplicity)
        self.batch_size = int(batch_size)
        self.device = device
        # capacity convention of the pipeline (as DeviceRWRSampler: B * (largest subgraph + 1)): the eigensolver sizes its
        # per-subgraph workspace as node_cap / batch_size
        self.node_cap = self.batch_size * (max(len(rp) - 1 for rp, _ in self.graphs) + 1)

    def __len__(self):
        return self.length

    def _convert_idx(self, idx):                                      # :326-329
        rp, _ = self.graphs[idx]
        return idx, int(np.argmax(np.diff(rp)))

    def _batch(self, lo, hi):
        import torch

        from .sampler import BatchedCSR

        B = self.batch_size
        node_off, edge_off, rows, cols, seeds = [0], [0], [], [], []
        for idx in range(lo, hi):
            rp, ci = self.graphs[idx]
            o = node_off[-1]
            rows.append(rp[1:] + edge_off[-1])
            cols.append(ci + o)
            seeds.append(self._convert_idx(idx)[1])
            node_off.append(o + len(rp) - 1)
            edge_off.append(edge_off[-1] + len(ci))
        for _ in range(hi - lo, B):                                   # padding: empty graphs
            node_off.append(node_off[-1])
            edge_off.append(edge_off[-1])
            seeds.append(0)
        n, e = node_off[-1], edge_off[-1]
        i32 = dict(dtype=torch.int32, device=self.device)
        row_ptr = torch.zeros(self.node_cap + 1, **i32)
        row_ptr[: n + 1] = torch.from_numpy(np.concatenate([[0]] + rows).astype(np.int32)).to(self.device)
        graph_id = torch.zeros(self.node_cap, **i32)
        graph_id[:n] = torch.repeat_interleave(torch.arange(B, dtype=torch.int32), torch.tensor(np.diff(node_off))).to(self.device)
        g = BatchedCSR(B, torch.tensor(node_off, **i32), torch.tensor(edge_off, **i32), torch.zeros(self.node_cap, **i32),
                       graph_id, row_ptr, torch.from_numpy(np.concatenate(cols).astype(np.int32)).to(self.device))
        g.seed_local = torch.tensor(seeds, **i32)
        g.edge_multiplicity = self.edge_multiplicity
        g.valid = hi - lo
        return g

    def __iter__(self):
        for lo in range(0, self.length, self.batch_size):
            g = self._batch(lo, min(lo + self.batch_size, self.length))
            yield g, g                                                # graph_q and graph_k are the same whole graph


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
    m = int(getattr(g, "edge_multiplicity", 1))
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
                 graphs=None, labels=None, edge_multiplicity=1, batch_size=32, run_seed=0, device="cuda"):
        super().__init__(dataset=dataset, rw_hops=rw_hops, subgraph_size=subgraph_size, restart_prob=restart_prob,
                         positional_embedding_size=positional_embedding_size, graphs=graphs,
                         edge_multiplicity=edge_multiplicity, batch_size=batch_size, device=device)
        if labels is None:
            raise ValueError("pass labels (graph_labels of the TU dataset)")
        self.labels = np.asarray(labels).astype(np.int64)
        assert len(self.labels) == self.length, "one label per graph"
        self.num_classes = int(self.labels.max()) + 1
        self.run_seed = run_seed
        self.sizes = np.array([len(rp) - 1 for rp, _ in self.graphs], dtype=np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.sizes)])
        self._pos = None                                               # [sum of nodes, P] on the device, every graph once
        self.posemb = None

    def _embed_all(self):
        import torch

        from .posemb import DevicePosEmb

        self.posemb = DevicePosEmb(self.batch_size, self.node_cap, self.positional_embedding_size, device=self.device,
                                   seed=self.run_seed, num_buffers=1)
        parts = []
        for lo in range(0, self.length, self.batch_size):
            idx = np.arange(lo, min(lo + self.batch_size, self.length))
            g = self._batch_of(idx)
            self.posemb(g)
            parts.append(g.pos_undirected[: int(self.first[idx[-1] + 1] - self.first[idx[0]])].clone())
        self._pos = torch.cat(parts)

    def _batch_of(self, idx):
        """GraphClassificationDataset._batch over an arbitrary list of graph indices (empty padding graphs)"""
        import torch

        from .sampler import BatchedCSR

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

    def make_batch(self, idx):
        import torch

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
        order = np.asarray(order, dtype=np.int64)
        for lo in range(0, len(order), self.batch_size):
            yield self.make_batch(order[lo:lo + self.batch_size])

    def check_status(self):
        if self.posemb is not None:
            self.posemb.check_status()
