"""Graph files of the reference's downstream datasets -> int32 CSR.

``<name>.edgelist`` / ``<name>.nodelabel`` as read by ``Edgelist._preprocess`` (gcc/datasets/data_util.py:61-110):
one "u v" pair per line, node ids re-indexed in order of first appearance; "node label" per line.  The reference then
inserts every pair in both directions (data_util.py:84-85) and its dataset class inserts both directions AGAIN
(graph_dataset.py:301-302), so its DGL graph is a multigraph in which every undirected edge of the file exists
``2 x (times the pair is listed, in either order)`` times per direction.  The HIP path keeps a simple CSR plus ONE
uniform multiplicity (gcc_gin_pass.edge_multiplicity); self loops are rejected, and so are files whose pairs repeat a
non-uniform number of times unless the caller asks for a multigraph: then every listing is its own parallel edge, a
repeated entry of a sorted CSR row (``multigraph_csr``), and only the uniform factor of the double insertion stays in
``edge_multiplicity``.

``read_ss_graph``: the ``<name>.graph`` / ``<name>.dict`` pairs of the similarity-search task (data_util.py:145-191).

``read_tudataset``: the raw TU Dortmund collection layout (``<NAME>_A.txt``, ``<NAME>_graph_indicator.txt``,
``<NAME>_graph_labels.txt``) that DGL's ``TUDataset`` downloads for ``create_graph_classification_dataset``
(data_util.py:47-58: imdb-binary, imdb-multi, rdt-b, rdt-5k, collab) -> the list of small graphs
``GraphClassificationDataset(graphs=...)`` takes, plus the graph labels."""
from __future__ import annotations

import numpy as np


class NonUniformMultiplicity(ValueError):
    """pairs of an edge list are listed a non-uniform number of times (``csr_from_pairs`` keeps ONE multiplicity)"""


def csr_from_pairs(pairs: np.ndarray, num_nodes: int):
    """pairs int64 [m, 2] (undirected, any order, repeats allowed) -> (row_ptr, col_idx, multiplicity)."""
    if (pairs[:, 0] == pairs[:, 1]).any():
        raise ValueError("self loops are not supported by the sampler contract (x2dgl.py:41-42 removes them)")
    lo, hi = pairs.min(axis=1), pairs.max(axis=1)
    key, counts = np.unique(lo * num_nodes + hi, return_counts=True)
    if counts.min() != counts.max():
        raise NonUniformMultiplicity("pairs repeat a non-uniform number of times: a general multigraph is not supported")
    u, v = key // num_nodes, key % num_nodes
    src = np.concatenate([u, v])
    dst = np.concatenate([v, u])
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    row_ptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.add.at(row_ptr, src + 1, 1)
    row_ptr = np.cumsum(row_ptr)
    if (np.diff(row_ptr) == 0).any():
        raise ValueError("isolated nodes (every node of an edge list has an edge; check the input)")
    return row_ptr.astype(np.int32), dst.astype(np.int32), int(counts[0])


def multigraph_csr(pairs: np.ndarray, weights: np.ndarray, num_nodes: int):
    """pairs int64 [m, 2] (undirected, any order; a pair may be listed more than once, its weights add up), weights int64 [m]
    (>= 1: parallel edges of the pair) -> (row_ptr, col_idx) int32 of the MULTIGRAPH: both directions, every parallel edge
    its own entry, rows sorted -- so the copies of a pair are adjacent (DGL's representation; what the sampler walks, the
    positional embedding counts and the encoders sum).  Only nodes with an edge may have an index below ``num_nodes``."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    weights = np.asarray(weights, dtype=np.int64).reshape(-1)
    if len(weights) != len(pairs):
        raise ValueError(f"{len(pairs)} pairs but {len(weights)} weights")
    if len(pairs) == 0:
        raise ValueError("no edges")
    if (weights < 1).any():
        raise ValueError("edge weights must be positive integers (the number of parallel edges)")
    if (pairs[:, 0] == pairs[:, 1]).any():
        raise ValueError("self loops are not supported by the sampler contract (x2dgl.py:41-42 removes them)")
    if pairs.min() < 0 or pairs.max() >= num_nodes:
        raise ValueError("node index out of range")
    if 2 * int(weights.sum()) >= 2 ** 31:
        raise ValueError("the expanded multigraph does not fit int32 entry offsets")
    src = np.repeat(np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([weights, weights]))
    dst = np.repeat(np.concatenate([pairs[:, 1], pairs[:, 0]]), np.concatenate([weights, weights]))
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    row_ptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=num_nodes), out=row_ptr[1:])
    if (np.diff(row_ptr) == 0).any():
        raise ValueError("isolated nodes (every node of the CSR needs an edge; check the input)")
    return row_ptr.astype(np.int32), dst.astype(np.int32)


def read_edgelist(edgelist_path: str, nodelabel_path: str = None, hindex: bool = False, multigraph: bool = False):
    """-> dict(row_ptr, col_idx, edge_multiplicity, node2id, y[, multigraph]).  ``edge_multiplicity`` is the number of copies of
    every edge in the graph the reference's NodeClassificationDataset builds (2 x listings).  ``multigraph``: pairs
    listed a NON-uniform number of times are expanded into repeated CSR entries (``multigraph_csr``: one parallel edge per
    listing) and ``edge_multiplicity`` is the 2 of the double insertion; uniformly listed files come out as without it."""
    node2id, pairs = {}, []
    with open(edgelist_path) as f:
        for line in f:
            if not line.strip():
                continue
            x, y = (int(t) for t in line.split()[:2])
            for n in (x, y):
                if n not in node2id:
                    node2id[n] = len(node2id)
            pairs.append((node2id[x], node2id[y]))
    num_nodes = len(node2id)
    pairs = np.asarray(pairs, dtype=np.int64)
    expanded = False
    try:
        row_ptr, col_idx, listed = csr_from_pairs(pairs, num_nodes)
    except NonUniformMultiplicity:
        if not multigraph:
            raise
        row_ptr, col_idx = multigraph_csr(pairs, np.ones(len(pairs), dtype=np.int64), num_nodes)
        listed, expanded = 1, True
    out = dict(row_ptr=row_ptr, col_idx=col_idx, edge_multiplicity=2 * listed, node2id=node2id, y=None)
    if multigraph:
        out["multigraph"] = expanded                 # the CSR holds repeated entries: consumers need DeviceGraph(multigraph=True)
    if nodelabel_path is not None:
        nodes, labels, label2id = [], [], {}
        with open(nodelabel_path) as f:
            for line in f:
                if not line.strip():
                    continue
                x, label = (int(t) for t in line.split()[:2])
                if label not in label2id:
                    label2id[label] = len(label2id)
                nodes.append(node2id[x])
                labels.append(label if hindex else label2id[label])
        if hindex:                                   # data_util.py:104-106
            median = np.median(labels)
            labels = [int(l > median) for l in labels]
        y = np.zeros((num_nodes, max(len(label2id), 1)), dtype=np.float32)
        y[nodes, labels] = 1
        out["y"] = y
    return out


def read_ss_graph(graph_path: str, dict_path: str, csr: bool = False):
    """``<name>.graph`` / ``<name>.dict`` of the similarity-search datasets (data/panther) as ``SSDataset._preprocess`` reads
    them (data_util.py:159-191): the first line of the graph file is a header; every other line is ``x y t``, a co-author pair
    and the number of joint papers, with ids re-indexed in order of first appearance; the dict file holds ``name<TAB>id``
    lines, and an id that no edge mentions gets the next free index.
    -> dict(node2id, name_dict {name: index}, pairs int64 [m, 2], weights int64 [m], num_nodes).  The reference's edge list
    is every pair ``weights`` times in both directions.
    ``csr``: adds ``row_ptr`` / ``col_idx`` (``multigraph_csr``: that edge list, parallel edges as repeated entries) over the
    ``num_graph_nodes`` nodes the graph file mentions, and ``edge_multiplicity`` = 2, the second insertion of every edge by
    the dataset class (graph_dataset.py:301-302).  Ids that occur only in the dict file were indexed after those nodes and
    stay out of the CSR, as in ``SSSingleDataset`` (data_util.py:111-143), whose graph has no node for them."""
    node2id, pairs, weights = {}, [], []
    with open(graph_path) as f:
        f.readline()
        for line in f:
            if not line.strip():
                continue
            x, y, t = (int(v) for v in line.split()[:3])
            for n in (x, y):
                if n not in node2id:
                    node2id[n] = len(node2id)
            pairs.append((node2id[x], node2id[y]))
            weights.append(t)
    num_graph_nodes = len(node2id)
    name_dict = {}
    with open(dict_path) as f:
        for line in f:
            if not line.strip():
                continue
            name, x = line.rstrip("\n").rsplit("\t", 1)
            x = int(x)
            if x not in node2id:
                node2id[x] = len(node2id)
            name_dict[name] = node2id[x]
    out = dict(node2id=node2id, name_dict=name_dict, pairs=np.asarray(pairs, dtype=np.int64).reshape(-1, 2),
               weights=np.asarray(weights, dtype=np.int64), num_nodes=len(node2id))
    if csr:
        out["num_graph_nodes"] = num_graph_nodes
        out["row_ptr"], out["col_idx"] = multigraph_csr(out["pairs"], out["weights"], num_graph_nodes)
        out["edge_multiplicity"] = 2
    return out


TU_NAMES = {"imdb-binary": "IMDB-BINARY", "imdb-multi": "IMDB-MULTI", "rdt-b": "REDDIT-BINARY",
            "rdt-5k": "REDDIT-MULTI-5K", "collab": "COLLAB"}                      # data_util.py:48-54


def read_tudataset(folder: str, name: str):
    """-> dict(graphs=[(row_ptr, col_idx), ...], graph_labels int64 [G], num_labels).  ``name`` is the reference's
    dataset name (``imdb-binary`` ...) or the TU name itself.  Nodes of a graph keep their file order (DGL builds each
    graph as the subgraph of its ascending node ids); labels are re-indexed 0..C-1 in ascending order of the file's
    values, as DGL's TUDataset does.  The adjacency must be symmetric without self loops or repeated entries."""
    import os

    tu = TU_NAMES.get(name, name)
    base = os.path.join(folder, tu + "_")
    edges = np.loadtxt(base + "A.txt", delimiter=",", dtype=np.int64, ndmin=2) - 1
    indicator = np.loadtxt(base + "graph_indicator.txt", dtype=np.int64, ndmin=1)
    labels = np.loadtxt(base + "graph_labels.txt", dtype=np.int64, ndmin=1)
    num_nodes = len(indicator)
    if (np.diff(indicator) < 0).any():
        raise ValueError("graph_indicator must be non-decreasing (nodes of a graph are contiguous in the TU format)")
    gids, first = np.unique(indicator, return_index=True)
    if len(gids) != len(labels):
        raise ValueError(f"{len(gids)} graphs in graph_indicator but {len(labels)} graph labels")
    src, dst = edges[:, 0], edges[:, 1]
    if len(src) and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= num_nodes):
        raise ValueError("node id out of range in A.txt")
    if (src == dst).any():
        raise ValueError("self loops are not supported by the sampler contract (x2dgl.py:41-42 removes them)")
    if (indicator[src] != indicator[dst]).any():
        raise ValueError("an edge connects two different graphs")
    key = src * num_nodes + dst
    if len(np.unique(key)) != len(key):
        raise ValueError("repeated adjacency entries: a general multigraph is not supported")
    if not np.array_equal(np.sort(key), np.sort(dst * num_nodes + src)):
        raise ValueError("the adjacency is not symmetric")
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    row_ptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.add.at(row_ptr, src + 1, 1)
    row_ptr = np.cumsum(row_ptr)
    bounds = np.append(first, num_nodes)
    graphs = []
    for g in range(len(gids)):
        lo, hi = int(bounds[g]), int(bounds[g + 1])
        rp = row_ptr[lo:hi + 1] - row_ptr[lo]
        graphs.append((rp.astype(np.int32), (dst[row_ptr[lo]:row_ptr[hi]] - lo).astype(np.int32)))
    values = np.unique(labels)
    return dict(graphs=graphs, graph_labels=np.searchsorted(values, labels).astype(np.int64), num_labels=len(values))


def write_tudataset(folder: str, name: str, graphs, graph_labels, sep: str = ", "):
    """The inverse of :func:`read_tudataset`: ``graphs`` = [(row_ptr, col_idx), ...] with ids local to each graph and
    ``graph_labels`` (any integers, one per graph) -> ``<TU name>_A.txt`` (one line ``u<sep>v`` per entry, 1-based global
    ids, rows in order), ``_graph_indicator.txt`` (graph ids 1..G) and ``_graph_labels.txt``.  -> the three paths."""
    import os

    tu = TU_NAMES.get(name, name)
    base = os.path.join(folder, tu + "_")
    if len(graphs) != len(graph_labels):
        raise ValueError(f"{len(graphs)} graphs but {len(graph_labels)} graph labels")
    os.makedirs(folder, exist_ok=True)
    src, dst, indicator, first = [], [], [], 0
    for g, (rp, ci) in enumerate(graphs):
        rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
        n = len(rp) - 1
        src.append(np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)) + first + 1)
        dst.append(ci + first + 1)
        indicator.append(np.full(n, g + 1, dtype=np.int64))
        first += n
    src = np.concatenate(src) if src else np.zeros(0, dtype=np.int64)
    dst = np.concatenate(dst) if dst else np.zeros(0, dtype=np.int64)
    with open(base + "A.txt", "w") as f:
        f.write("".join(f"{u}{sep}{v}\n" for u, v in zip(src.tolist(), dst.tolist())))
    with open(base + "graph_indicator.txt", "w") as f:
        f.write("".join(f"{x}\n" for x in (np.concatenate(indicator).tolist() if indicator else [])))
    with open(base + "graph_labels.txt", "w") as f:
        f.write("".join(f"{int(x)}\n" for x in graph_labels))
    return base + "A.txt", base + "graph_indicator.txt", base + "graph_labels.txt"


def read_lscc(path: str):
    """The text layout of the pre-training networks as ``yuxiao_kdd17_graph_to_dgl`` reads it (x2dgl.py:30-47): a ``<word> n``
    line, ``n`` vertex lines (zero-based index and raw id: skipped), a ``<word> m`` line, then ``m`` lines ``u v w`` (``w`` is
    read and dropped, as there).  -> (n, pairs int32 [m, 2]): the lines as they stand, self loops and repeats included -- what
    ``gcc_amd.graph_build`` takes.  The file is parsed as one array: no Python loop per line."""
    with open(path, "rb") as f:
        data = f.read()
    ends = np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10)          # the line ends

    def count_of(line, what):
        words = line.split()
        if len(words) < 2 or not words[1].lstrip(b"-").isdigit():
            raise ValueError(f"{path}: expected a `<word> {what}` line, found {line[:40]!r}")
        return int(words[1])

    if len(ends) < 1:
        raise ValueError(f"{path}: truncated: no `<word> n` line")
    n = count_of(data[:ends[0]], "n")
    if n < 0 or len(ends) < n + 2:
        raise ValueError(f"{path}: truncated: {n} vertex lines and a `<word> m` line announced, the file has {len(ends)} lines")
    m = count_of(data[ends[n] + 1:ends[n + 1]], "m")
    try:
        body = np.array(data[ends[n + 1] + 1:].split(), dtype=np.int64)
    except ValueError as err:
        raise ValueError(f"{path}: an edge line holds something other than integers ({err})") from None
    if m < 0 or body.size < 3 * m:
        raise ValueError(f"{path}: truncated: {m} edge lines `u v w` announced, {body.size // 3} complete ones found")
    pairs = body[:3 * m].reshape(m, 3)[:, :2]
    if m and (pairs.min() < -2 ** 31 or pairs.max() >= 2 ** 31):
        raise ValueError(f"{path}: node ids must fit int32")
    return n, np.ascontiguousarray(pairs, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------
# DGL graph files (``data/small.bin``): what ``dgl.data.utils.save_graphs`` / ``load_graphs`` / ``load_labels`` of
# dgl 0.4.x write and read -- graph_dataset.py:26-29 (worker_init_fn), graph_dataset.py:58-60 (graph_sizes label),
# x2dgl.py:119-131 (the converter that produces the pre-training corpus).
#
# FORMAT STATUS: DGL-recalled, parity UNPINNED.  DGL is neither vendored in /root/reference nor installable here, and
# the reference ships no .bin file, so the container layout below is a restatement from memory of dgl 0.4.3's
# src/graph/graph_serialize.cc and the DLPack tensor blobs of src/runtime/ndarray.cc; the reader checks every magic
# number and size it relies on and raises on the first mismatch instead of guessing.  Layout (little endian):
#
#   0     u64 magic 0xDD2E4FF046B4A13F | u64 version (1) | u64 graph type (1 = immutable) | zero padding to 4096
#   4096  u64 num_graph
#         vector<u64> graph_offsets   (dmlc vector = u64 count + elements: absolute file offset of each graph)
#         vector<u64> num_nodes, vector<u64> num_edges
#         vector<pair<string, tensor>> labels          (string = u64 length + bytes; here: "graph_sizes")
#   per graph, at its offset: tensor indptr[n+1], tensor indices[nnz], tensor edge_ids[nnz]  (the IN-CSR, int64),
#         vector<pair<string, tensor>> node data, vector<pair<string, tensor>> edge data
#   tensor = u64 magic 0xDD5E40F096B4A13F | u64 reserved | i32 device_type (1 = CPU) | i32 device_id | i32 ndim |
#            u8 dtype code (0 int, 1 uint, 2 float) | u8 bits | u16 lanes | i64 shape[ndim] | i64 nbytes | data
_DGL_MAGIC = 0xDD2E4FF046B4A13F
_NDARRAY_MAGIC = 0xDD5E40F096B4A13F
_DT_CODES = {0: "i", 1: "u", 2: "f"}


class _Reader:
    def __init__(self, buf, name):
        self.b, self.o, self.name = memoryview(buf), 0, name

    def take(self, fmt):
        import struct

        size = struct.calcsize("<" + fmt)
        if self.o + size > len(self.b):
            raise ValueError(f"{self.name}: truncated at byte {self.o}")
        v = struct.unpack_from("<" + fmt, self.b, self.o)
        self.o += size
        return v if len(v) > 1 else v[0]

    def u64_vector(self):
        n = self.take("Q")
        if n > (len(self.b) - self.o) // 8:
            raise ValueError(f"{self.name}: vector of {n} entries does not fit the file (offset {self.o})")
        v = np.frombuffer(self.b, dtype="<u8", count=n, offset=self.o).copy()
        self.o += 8 * n
        return v

    def string(self):
        n = self.take("Q")
        if n > 4096:
            raise ValueError(f"{self.name}: implausible string length {n} at byte {self.o}")
        s = bytes(self.b[self.o:self.o + n]).decode()
        self.o += n
        return s

    def tensor(self):
        magic, _reserved = self.take("QQ")
        if magic != _NDARRAY_MAGIC:
            raise ValueError(f"{self.name}: tensor magic {magic:#x} at byte {self.o - 16} (expected {_NDARRAY_MAGIC:#x})")
        dev_type, _dev_id, ndim = self.take("iii")
        code, bits, lanes = self.take("BBH")
        if dev_type != 1 or lanes != 1 or code not in _DT_CODES or ndim < 0 or ndim > 8:
            raise ValueError(f"{self.name}: unsupported tensor header (device {dev_type}, dtype {code}/{bits}/{lanes}, ndim {ndim})")
        shape = [self.take("q") for _ in range(ndim)]
        nbytes = self.take("q")
        count = int(np.prod(shape)) if ndim else 1
        if nbytes != count * bits // 8 or self.o + nbytes > len(self.b):
            raise ValueError(f"{self.name}: tensor of shape {shape} with {nbytes} bytes at byte {self.o}")
        a = np.frombuffer(self.b, dtype=f"<{_DT_CODES[code]}{bits // 8}", count=count, offset=self.o).reshape(shape).copy()
        self.o += nbytes
        return a

    def named_tensors(self):
        return {self.string(): self.tensor() for _ in range(self.take("Q"))}


def _dgl_header(r):
    magic, version, gtype = r.take("QQQ")
    if magic != _DGL_MAGIC:
        raise ValueError(f"{r.name}: not a DGL graph file (magic {magic:#x}, expected {_DGL_MAGIC:#x})")
    if version != 1 or gtype != 1:
        raise ValueError(f"{r.name}: DGL graph file version {version} / graph type {gtype}; only the dgl 0.4.x immutable-graph "
                         "container (version 1, type 1) is understood")
    r.o = 4096
    num = r.take("Q")
    offsets, nodes, edges = r.u64_vector(), r.u64_vector(), r.u64_vector()
    if not (len(offsets) == len(nodes) == len(edges) == num):
        raise ValueError(f"{r.name}: graph table sizes disagree ({num}, {len(offsets)}, {len(nodes)}, {len(edges)})")
    return offsets, nodes, edges, r.named_tensors()


def read_dgl_labels(path: str) -> dict:
    """``dgl.data.utils.load_labels(path)`` (graph_dataset.py:58-60): the label dict only, without touching the graphs."""
    with open(path, "rb") as f:
        r = _Reader(f.read(), path)
    return _dgl_header(r)[3]


def read_dgl_graphs(path: str, idx_list=None, validate: bool = True):
    """``dgl.data.utils.load_graphs(path, idx_list)`` (graph_dataset.py:26-29) -> ([(row_ptr, col_idx) int32, ...], labels).
    The stored structure is the in-CSR; the sampler contract (x2dgl.py:39-62: symmetric, no self loops, no duplicates,
    no isolated nodes -- so in-CSR == out-CSR) is checked per graph unless ``validate=False``."""
    from .graphgen import check_contract

    with open(path, "rb") as f:
        r = _Reader(f.read(), path)
    offsets, nodes, edges, labels = _dgl_header(r)
    graphs = []
    for i in (range(len(offsets)) if idx_list is None else idx_list):
        r.o = int(offsets[i])
        indptr, indices, _edge_ids = r.tensor(), r.tensor(), r.tensor()
        r.named_tensors()                                   # node data (x2dgl.py:122 clears it)
        r.named_tensors()                                   # edge data
        if len(indptr) != nodes[i] + 1 or len(indices) != edges[i] or indptr[-1] != edges[i]:
            raise ValueError(f"{path}: graph {i}: CSR of {len(indptr) - 1} nodes / {len(indices)} edges, table says {nodes[i]} / {edges[i]}")
        if edges[i] >= 2 ** 31 or nodes[i] >= 2 ** 31:
            raise ValueError(f"{path}: graph {i} does not fit int32 ids")
        rp, ci = indptr.astype(np.int32), indices.astype(np.int32)
        if validate:
            # DGL does not promise sorted rows (an in-CSR materialised from COO input keeps insertion order and carries a
            # permutation in edge_ids); the sampler does.  One vectorised pass over ALL rows: a descent is only allowed
            # where a new row starts.
            if len(ci) > 1:
                descent = np.flatnonzero(np.diff(ci.astype(np.int64)) <= 0) + 1       # positions whose predecessor is >= them
                starts = np.zeros(len(ci) + 1, dtype=bool)
                starts[rp[:-1]] = True
                if not np.all(starts[descent]):
                    order = np.lexsort((ci, np.repeat(np.arange(len(rp) - 1), np.diff(rp))))
                    ci = ci[order]
            check_contract(rp, ci)
        graphs.append((rp, ci))
    if idx_list is None and "graph_sizes" in labels and len(labels["graph_sizes"]) != len(graphs):
        raise ValueError(f"{path}: label graph_sizes has {len(labels['graph_sizes'])} entries for {len(graphs)} graphs "
                         "(x2dgl.py:120,129-131 writes one node count per graph)")
    return graphs, labels


def write_dgl_graphs(path: str, graphs, labels: dict = None):
    """The inverse of :func:`read_dgl_graphs` (``save_graphs(filename, g_list, labels)``, x2dgl.py:129-131) for symmetric
    CSR graphs.  Same format status: DGL-recalled, unpinned -- it exists so that corpora can be prepared without DGL and
    so that the tests can round-trip the reader."""
    import struct

    def tensor(a):
        a = np.ascontiguousarray(a)
        code = {"i": 0, "u": 1, "f": 2}[a.dtype.kind]
        head = struct.pack("<QQiiiBBH", _NDARRAY_MAGIC, 0, 1, 0, a.ndim, code, a.dtype.itemsize * 8, 1)
        return head + struct.pack(f"<{a.ndim}q", *a.shape) + struct.pack("<q", a.nbytes) + a.astype(a.dtype.newbyteorder("<")).tobytes()

    def named(d):
        out = struct.pack("<Q", len(d))
        for k, v in d.items():
            kb = k.encode()
            out += struct.pack("<Q", len(kb)) + kb + tensor(np.asarray(v))
        return out

    def vec(v):
        return struct.pack("<Q", len(v)) + np.asarray(v, dtype="<u8").tobytes()

    blobs = []
    for rp, ci in graphs:
        rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
        blobs.append(tensor(rp) + tensor(ci) + tensor(np.arange(len(ci), dtype=np.int64)) + named({}) + named({}))
    nodes = [len(rp) - 1 for rp, _ in graphs]
    edges = [len(ci) for _, ci in graphs]
    lab = named(labels or {})
    table = 4096 + 8 + 3 * (8 + 8 * len(graphs)) + len(lab)
    offsets, o = [], table
    for b in blobs:
        offsets.append(o)
        o += len(b)
    with open(path, "wb") as f:
        f.write(struct.pack("<QQQ", _DGL_MAGIC, 1, 1).ljust(4096, b"\0"))
        f.write(struct.pack("<Q", len(graphs)) + vec(offsets) + vec(nodes) + vec(edges) + lab)
        for b in blobs:
            f.write(b)
