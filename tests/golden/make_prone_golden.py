"""Generates tests/golden/prone_<name>.npz by EXECUTING THE REFERENCE'S OWN ``ProNE(d).train(G)`` (gcc/models/emb/prone.py, loaded
by path; no text of it is copied).  The reference calls ``randomized_svd(..., random_state=None)``; here ``prone.randomized_svd``
is wrapped to pass ``random_state=np.random.RandomState(seed)`` and runs three times per graph:

    lu      as the reference calls it (sklearn normalises the power iterations by LU for n_iter = 5)
    qr      with power_iteration_normalizer="QR"
    gesvd   with svd_lapack_driver="gesvd"

Every file holds the edges (u < v), n, d, the seed and the three embeddings in node-id rows, zero for a node id that no
edge names (gcc/tasks/node_classification.py builds its feature matrix that way).  The graph G gets its nodes in ascending id
order, so the reference's rows are the node ids in that order.  Omega in node-id order is sklearn's draw for the seed,
``np.random.RandomState(seed).normal(size=(n, d + 10))``, which tests/prone_reference.py draws again (RandomState's stream is
frozen); ``hub`` stores its Omega, because a node id that no edge names gets a row of a second stream there, which nothing may read.

Conditions the script asserts, rejecting a candidate graph (the next graph seed is tried):
  * the smallest relative gap (s_i - s_{i+1}) / s_i among the d singular values of BOTH decompositions is >= 1e-3 in all three
    runs, so that no two columns can rotate into each other between implementations;
  * the factorised matrix has rank >= d + 10 (the hub graph included), so the range finder keeps full rank;
  * ``task`` (two planted communities, the labels): every row of the lu embedding is closer to its own class centroid than to the
    other's by at least 0.25 in cosine similarity, so that a perturbation of 1e-6 cannot move a prediction.

Graphs: G(n, p) plus the path 0-1-...-(n-1) (every id is named in ascending order, which makes gcc_amd.ingest.read_edgelist's ids
the file's own).  ``hub``: ids 7 and 150 are named by no edge; node 0 is joined to every other named node (297 neighbours).

    python tests/golden/make_prone_golden.py
"""
import importlib.util
import os
import sys

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference/gcc/models/emb/prone.py"
# name -> n, d, edge probability
FIXTURES = {"n201d16": (201, 16, 0.05), "n120d64": (120, 64, 0.3), "n74d64": (74, 64, 0.4), "n300d6": (300, 6, 0.03),
            "n40d2": (40, 2, 0.15), "hub": (300, 8, 0.02), "task": (100, 8, None)}
ISOLATED = {"hub": (7, 150)}
MIN_GAP = 1e-3
MIN_MARGIN = 0.25


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_prone", REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def graph(name, n, p, rng):
    """-> (edges [m, 2] with u < v, labels or None)"""
    iso = set(ISOLATED.get(name, ()))
    ids = [i for i in range(n) if i not in iso]
    edges = {(a, b) for a, b in zip(ids[:-1], ids[1:])}
    labels = None
    if name == "task":
        labels = (np.arange(n) >= n // 2).astype(np.int64)
        prob = np.where(labels[:, None] == labels[None, :], 0.3, 0.01)
    else:
        prob = np.full((n, n), p)
    draw = rng.random_sample((n, n))
    for u in ids:
        for v in ids:
            if u < v and draw[u, v] < prob[u, v]:
                edges.add((u, v))
    if name == "hub":
        edges |= {(0, v) for v in ids[1:]}
    return np.array(sorted(edges), dtype=np.int32), labels


def run_reference(ref, edges, ids, d, seed, **kw):
    """-> (embedding in G's node order, the singular values of the two decompositions)"""
    G = nx.Graph()
    G.add_nodes_from(ids)
    G.add_edges_from(edges.tolist())
    seen = {}
    inner_rsvd, inner_svd = ref.randomized_svd, ref.linalg.svd

    def rsvd(m, n_components, n_iter, random_state):
        out = inner_rsvd(m, n_components=n_components, n_iter=n_iter, random_state=np.random.RandomState(seed), **kw)
        seen["rand"] = out[1].copy()
        return out

    class Linalg:
        @staticmethod
        def svd(m, **kws):
            out = inner_svd(m, **kws)
            seen["dense"] = out[1][:d].copy()
            return out

    ref.randomized_svd, keep = rsvd, ref.linalg
    ref.linalg = Linalg
    try:
        emb = ref.ProNE(d).train(G)
    finally:
        ref.randomized_svd, ref.linalg = inner_rsvd, keep
    return np.asarray(emb), seen


def factor_rank(edges, n):
    from gcc_amd.prone import node_terms

    a = np.zeros((n, n), dtype=bool)
    a[edges[:, 0], edges[:, 1]] = a[edges[:, 1], edges[:, 0]] = True
    row_ptr = np.concatenate([[0], np.cumsum(a.sum(1))])
    col_idx = np.nonzero(a)[1]
    _, r, c = node_terms(row_ptr, col_idx)
    with np.errstate(invalid="ignore"):
        f = np.where(a, r[:, None] + c[None, :], 0.0)
    return int(np.linalg.matrix_rank(f))


def make(ref, name):
    n, d, p = FIXTURES[name]
    iso = ISOLATED.get(name, ())
    ids = [i for i in range(n) if i not in iso]
    for graph_seed in range(100):
        seed = 1000 + graph_seed
        edges, labels = graph(name, n, p, np.random.RandomState(graph_seed))
        if factor_rank(edges, n) < d + 10:
            continue
        runs = {"lu": {}, "qr": dict(power_iteration_normalizer="QR"), "gesvd": dict(svd_lapack_driver="gesvd")}
        embs, gap = {}, np.inf
        for key, kw in runs.items():
            emb, seen = run_reference(ref, edges, ids, d, seed, **kw)
            full = np.zeros((n, d))
            full[ids] = emb
            embs[key] = full
            for s in seen.values():
                gap = min(gap, float(((s[:-1] - s[1:]) / s[:-1]).min()))
        if gap < MIN_GAP or not all(np.isfinite(e).all() for e in embs.values()):
            continue
        margin = -1.0
        if labels is not None:
            cent = np.stack([embs["lu"][labels == c].mean(0) for c in (0, 1)])
            cent /= np.linalg.norm(cent, axis=1, keepdims=True)
            cos = embs["lu"] @ cent.T
            margin = float((cos[np.arange(n), labels] - cos[np.arange(n), 1 - labels]).min())
            if margin < MIN_MARGIN:
                continue
        omega = np.random.RandomState(seed + 7).normal(size=(n, d + 10))
        omega[ids] = np.random.RandomState(seed).normal(size=(len(ids), d + 10))
        extra = {} if labels is None else dict(labels=labels)
        if iso:
            extra["omega"] = omega
        np.savez(os.path.join(HERE, f"prone_{name}.npz"), edges=edges, n=n, d=d, seed=seed, graph_seed=graph_seed,
                 emb_lu=embs["lu"], emb_qr=embs["qr"], emb_gesvd=embs["gesvd"], min_gap=gap, margin=margin, **extra)
        print(f"{name}: n {n} d {d} edges {len(edges)} graph seed {graph_seed} min gap {gap:.3g} margin {margin:.3g}")
        return
    raise SystemExit(f"{name}: no candidate graph met the conditions")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    reference = load_reference()
    for fixture_name in (sys.argv[1:] or FIXTURES):
        make(reference, fixture_name)
