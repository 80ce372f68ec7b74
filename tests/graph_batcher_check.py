"""gcc_pack_graphs against the host batcher, shared by the emulator tier (tests/test_graph_batcher_emu.py) and the GPU tier
(tests/test_graph_batcher_gpu.py): the same corpus, the same batches, the same exact comparisons; only the library, the
pointer function and the device differ.

The reference of every comparison is ``GraphClassificationDatasetLabeled(batcher="host")``: ``_batch_of``, the host gather of
the positional rows and ``_expand_multiplicity``.  Everything is compared exactly (integers equal, positional rows bit-equal).

Corpus: node counts on both sides of the wave (63 / 64 / 65), of the row tile (255 / 256 / 257) and of several tiles (1025), the
degenerate graphs (1 node and no edge, 2 nodes), and a star whose hub row (2,099 entries) is longer than a tile of 2,048 entries."""
import ctypes
import functools

import numpy as np
import torch

from gcc_amd import _cabi
from gcc_amd.datasets import DeviceGraphCorpus, GraphClassificationDatasetLabeled

SIZES = (1, 2, 9, 63, 64, 65, 255, 256, 257, 1025, 5)
STAR = 2100                                   # graph 11: the largest graph
SMALL = (0, 1, 2, 3, 4, 5, 10)                # the graphs of the 1024-wide batch
GUARD, SENTINEL = 16, 0x5A5A5A5A


def ring_with_chords(n, seed):
    """(row_ptr, col_idx) of a ring of n nodes plus about n / 2 random chords: simple, symmetric, rows sorted"""
    rng = np.random.RandomState(seed)
    pairs = set()
    if n == 2:
        pairs.add((0, 1))
    elif n > 2:
        pairs = {(i, (i + 1) % n) if i < (i + 1) % n else ((i + 1) % n, i) for i in range(n)}
        for _ in range(n // 2):
            a, b = sorted(int(x) for x in rng.randint(0, n, 2))
            if a != b:
                pairs.add((a, b))
    return csr_of(pairs, n)


def csr_of(pairs, n):
    adj = [[] for _ in range(n)]
    for a, b in pairs:
        adj[a].append(b)
        adj[b].append(a)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum([len(r) for r in adj])
    ci = np.array([c for r in adj for c in sorted(r)], dtype=np.int64)
    return rp, ci


@functools.lru_cache(maxsize=None)
def shape_corpus():
    graphs = [ring_with_chords(n, 100 + i) for i, n in enumerate(SIZES)]
    graphs.append(csr_of({(7, i) for i in range(STAR) if i != 7}, STAR))       # a star around node 7
    labels = [i % 3 for i in range(len(graphs))]
    return graphs, labels


def pos_table(total, P):
    """distinct bit patterns everywhere (a float32 view of a counter, so rows cannot be confused and no NaN compare is needed)"""
    return torch.from_numpy((np.arange(total * P, dtype=np.int64) % (1 << 22) + 0x3F000000).astype(np.int32).view(np.float32)
                            .reshape(total, P).copy())


SHAPE_BATCHES = {
    "one": [9],
    "lone_then_padding": [3, -1, -1, -1],
    "all_padding": [-1, -1, -1, -1],
    "repeated": [5, 5, 2, 5],
    "largest_first": [11, 9, 8, 7, 6, 5, 4, 3, 2, 10, 1, 0],
    "smallest_first": [0, 1, 10, 2, 3, 4, 5, 6, 7, 8, 9, 11],
    "largest_at_capacity": [11, 11, 11, 11],
    "wide_1024": [SMALL[i] for i in np.random.RandomState(5).randint(0, len(SMALL), 1024)],
}


@functools.lru_cache(maxsize=None)
def host_dataset(B, expand, P):
    """the yardstick: the host batcher on the CPU, with an injected table of positional rows"""
    graphs, labels = shape_corpus()
    ds = GraphClassificationDatasetLabeled(graphs=graphs, labels=labels, positional_embedding_size=P, edge_multiplicity=expand,
                                           batch_size=B, device="cpu", batcher="host")
    ds._pos = pos_table(int(ds.first[-1]), P)
    return ds


def host_reference(B, expand, P, idx):
    """What the host code gives for the batch ``idx`` (length B, < 0 or out of range = padding, anywhere in the batch):
    make_batch over the real graphs, with the empty padding graphs put back at their places."""
    ds = host_dataset(B, expand, P)
    G = ds.length
    slots = [b for b, i in enumerate(idx) if 0 <= i < G]
    real = [idx[b] for b in slots]
    g, lab = ds.make_batch(real)
    n, e = int(g.node_off[len(real)]), int(g.edge_off[len(real)])
    sizes, ecount = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    sizes[slots] = np.diff(g.node_off[: len(real) + 1].numpy())
    ecount[slots] = np.diff(g.edge_off[: len(real) + 1].numpy())
    seeds, labels = np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    seeds[slots] = g.seed_local[: len(real)].numpy()
    labels[slots] = lab[: len(real)].numpy()
    return dict(node_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                edge_off=np.concatenate([[0], np.cumsum(ecount)]).astype(np.int32),
                graph_id=np.asarray(slots, dtype=np.int32)[g.graph_id[:n].numpy()] if n else np.zeros(0, np.int32),
                row_ptr=g.row_ptr[: n + 1].numpy(), col_idx=g.col_idx[:e].numpy(), seed_local=seeds, labels=labels,
                pos=g.pos_undirected[:n].numpy().view(np.int32), n=n, e=e)


class Packer:
    """gcc_pack_graphs through ``lib`` with tensors on ``device``; every output buffer is followed by guard words"""

    def __init__(self, lib, ptr, device):
        self.lib, self.ptr, self.device = lib, ptr, device
        self._corpora = {}

    def corpus(self, P):
        if P not in self._corpora:
            graphs, labels = shape_corpus()
            c = DeviceGraphCorpus(graphs, 4, labels=labels, pos_dim=P, device=self.device, num_buffers=1, lib=self.lib,
                                  ptr=self.ptr)
            c.set_pos(pos_table(int(c.first[-1]), P).to(self.device))
            self._corpora[P] = c
        return self._corpora[P]

    def _guarded(self, n, dtype=torch.int32):
        t = torch.full((n + GUARD,), -7, dtype=torch.int32, device=self.device)
        t[n:] = SENTINEL
        return t if dtype == torch.int32 else t.view(torch.float32)

    def __call__(self, idx, expand, P, node_cap, edge_cap, with_labels=True):
        """-> (rc, outputs as numpy with the guard words cut off, status, guards intact)"""
        c = self.corpus(P)
        B = len(idx)
        idx_dev = torch.tensor(idx, dtype=torch.int32, device=self.device)
        lens = dict(node_off=B + 1, edge_off=B + 1, graph_id=node_cap, row_ptr=node_cap + 1, col_idx=edge_cap, seed_local=B,
                    labels=B, pos=node_cap * P)
        buf = {k: self._guarded(v) for k, v in lens.items()}
        status = torch.zeros(1 + GUARD, dtype=torch.int32, device=self.device)
        status[1:] = SENTINEL
        out = _cabi.GccBatchOut(node_off=self.ptr(buf["node_off"]), edge_off=self.ptr(buf["edge_off"]), parent_nid=None,
                                graph_id=self.ptr(buf["graph_id"]), row_ptr=self.ptr(buf["row_ptr"]),
                                col_idx=self.ptr(buf["col_idx"]), node_cap=node_cap, edge_cap=edge_cap)
        rc = self.lib.gcc_pack_graphs(ctypes.byref(c.c), self.ptr(idx_dev), B, ctypes.byref(out), self.ptr(buf["pos"]),
                                      self.ptr(buf["seed_local"]), self.ptr(buf["labels"]) if with_labels else None, expand,
                                      self.ptr(status), _cabi.raw_stream(self.device))
        got = {k: v.cpu().numpy() for k, v in buf.items()}
        st = status.cpu().numpy()
        intact = bool((st[1:] == SENTINEL).all()) and all(bool((got[k][lens[k]:] == SENTINEL).all()) for k in lens)
        return rc, {k: got[k][: lens[k]] for k in lens}, int(st[0]), intact


def assert_equals_host(got, ref, B, P):
    n, e = ref["n"], ref["e"]
    for key in ("node_off", "edge_off", "seed_local", "labels"):
        assert np.array_equal(got[key], ref[key]), key
    assert np.array_equal(got["graph_id"][:n], ref["graph_id"]), "graph_id"
    assert np.array_equal(got["row_ptr"][: n + 1], ref["row_ptr"]), "row_ptr"
    assert np.array_equal(got["col_idx"][:e], ref["col_idx"]), "col_idx"
    assert np.array_equal(got["pos"][: n * P].reshape(n, P), ref["pos"]), "pos"


def check_shape(pack, name, expand, P):
    """one batch of SHAPE_BATCHES: equal to the host batcher, status clean, guards intact"""
    idx = SHAPE_BATCHES[name]
    B = len(idx)
    ref = host_reference(B, expand, P, idx)
    spare = 0 if name == "largest_at_capacity" else 5             # zero spare capacity: the last row is the last word
    rc, got, status, intact = pack(idx, expand, P, ref["n"] + spare, max(ref["e"] + spare, 1))
    assert rc == 0, pack.lib.gcc_last_error().decode()
    assert status == 0 and intact
    assert_equals_host(got, ref, B, P)


def check_overflow(pack, which, expand, P):
    """graphs 9 (1,025 nodes), 8, 7, 6 with a capacity that ends inside graph 7: the status bit is set, nothing is written past
    any buffer, the offsets are monotone and within capacity, and what is left is the batch of the graphs that fit"""
    idx = [9, 8, 7, 6]
    full = host_reference(4, expand, P, idx)
    fit = host_reference(4, expand, P, [9, 8, -1, -1])
    if which == "node":
        node_cap, edge_cap = int(full["node_off"][2]) + 10, full["e"] + 3
    else:
        node_cap, edge_cap = full["n"] + 3, int(full["edge_off"][2]) + 10
    rc, got, status, intact = pack(idx, expand, P, node_cap, edge_cap)
    assert rc == 0 and intact
    assert status == (_cabi.STATUS_PACK_NODE_OVERFLOW if which == "node" else _cabi.STATUS_PACK_EDGE_OVERFLOW)
    for key, cap in (("node_off", node_cap), ("edge_off", edge_cap)):
        assert (np.diff(got[key]) >= 0).all() and got[key][0] == 0 and got[key][-1] <= cap, key
    n = int(got["node_off"][-1])
    assert (np.diff(got["row_ptr"][: n + 1]) >= 0).all() and got["row_ptr"][n] == got["edge_off"][-1]
    assert_equals_host(got, fit, 4, P)


def check_bad_index(pack, P):
    idx = [2, 99, 5, -7]
    rc, got, status, intact = pack(idx, 1, P, 200, 2000)
    assert rc == 0 and intact and status == _cabi.STATUS_PACK_BAD_INDEX
    assert_equals_host(got, host_reference(4, 1, P, [2, -1, 5, -1]), 4, P)


def check_refusals(pack):
    """argument errors are refused by name and launch nothing"""
    rc, _, status, intact = pack([0] * (_cabi.PACK_GRAPHS_MAX_BATCH + 1), 1, 2, 2000, 10)
    assert rc < 0 and intact and status == 0
    assert "GCC_PACK_GRAPHS_MAX_BATCH" in pack.lib.gcc_last_error().decode()
    rc, _, status, intact = pack([0], 0, 2, 10, 10)
    assert rc < 0 and "expand" in pack.lib.gcc_last_error().decode()
    rc, got, status, intact = pack([2], 1, 2, 20, 100, with_labels=False)       # labels_out may be NULL: left alone
    assert rc == 0 and status == 0 and (got["labels"] == -7).all()
