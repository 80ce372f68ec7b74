"""Generates tests/golden/graphwave_<name>.npz by EXECUTING THE REFERENCE'S OWN ``GraphWave(d).train(G)``
(gcc/models/emb/graphwave.py and its ``_graphwave`` package, loaded from the reference tree; no text of it is copied).

To import it on a current stack the script, at run time only: puts an empty ``seaborn`` module into ``sys.modules`` (used by the
plotting helpers alone); registers bare package modules ``gcc``, ``gcc.models`` and ``gcc.models.emb`` with only ``__path__`` set
(the package's own ``__init__`` imports DGL); restores two aliases SciPy 1.15 dropped, ``scipy.sum`` as a left fold with ``+`` and
an ``A`` property equal to ``toarray()`` on the sparse base classes; and runs matplotlib under ``Agg``.

Every file holds the edges (u < v; a parallel edge is a repeated row), the node-id count n_rows, d, the reference's table in
node-id rows (zero for an id that no edge names), for some files the two thresholded heat matrices ``heat_print`` over the
live nodes, and ``variant_distance``, the larger of
  (a) the largest distance between the reference's table and its own table on three random relabellings of the nodes, mapped
      back (``relabel_distance``), and
  (b) the distance of the reference's table from the same formulas evaluated in ``np.longdouble``, the taus and time points
      taken as the float64 values the reference uses (``longdouble_distance``): the errors of the coefficients and of H reach the
      table multiplied by t <= 100, so this is what float64 can deliver.

Conditions the script asserts, trying the next graph seed when one fails:
  * no pre-threshold entry of either heat matrix (gcc_amd.graphwave.heat_numpy) lies within a relative 1e-6 of the threshold, so
    no entry can fall on different sides in two float64 implementations;
  * over the whole set: in at least one fixture the threshold zeroes more than 5 % of the entries that were non-zero, some of them
    negative (``zeroed`` / ``zeroed_negative`` are stored per file);
  * ``task`` (nine cliques of 5 joined in a ring by paths of 6; label = clique member / path member): sklearn's one-vs-rest
    LogisticRegression(C=1000) on the reference's table scores micro-F1 1.0 in all ten folds of the task's split, and every
    held-out decision value is at least 1.0 from zero, so a perturbation of 1e-6 cannot move a prediction.  The fixture is 16
    wide: at d = 8 (the time points 0 and 100 alone) the worst fold scores 0.6 on the reference's own table; at 16 the smallest
    decision value is 3.6.

Graphs: the path through the ids in ascending order plus random chords (every id is named in ascending order, which makes
gcc_amd.ingest.read_edgelist's ids the file's own).

    python tests/golden/make_graphwave_golden.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"
# name -> n_rows, d, chords, keep heat_print
FIXTURES = {"n40d4": (40, 4, 8, False), "n65d8": (65, 8, 20, True), "n257d64": (257, 64, 120, False), "n300d16": (300, 16, 4, True),
            "hub300d8": (300, 8, 40, False), "multi130d32": (130, 32, 60, False), "n40d256": (40, 256, 8, False),
            "task": (99, 16, 0, False)}
ISOLATED = {"hub300d8": (7, 150)}
EDGE_GAP = 1e-6
MIN_DECISION = 1.0


def load_reference():
    import matplotlib

    matplotlib.use("Agg")
    import scipy
    import scipy.sparse as sp

    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    for name, sub in (("gcc", "gcc"), ("gcc.models", "gcc/models"), ("gcc.models.emb", "gcc/models/emb")):
        mod = types.ModuleType(name)
        mod.__path__ = [os.path.join(REFERENCE, sub)]
        sys.modules[name] = mod
    if not hasattr(scipy, "sum"):
        def left_fold(items):
            total = items[0]
            for item in items[1:]:
                total = total + item
            return total
        scipy.sum = left_fold
    for base in (sp.spmatrix, getattr(sp, "sparray", None)):
        if base is not None and not hasattr(base, "A"):
            base.A = property(lambda self: self.toarray())
    import importlib

    return importlib.import_module("gcc.models.emb.graphwave")


def graph(name, n, chords, rng):
    """-> (edges [m, 2] with u < v, a parallel edge repeated; labels or None)"""
    iso = set(ISOLATED.get(name, ()))
    ids = [i for i in range(n) if i not in iso]
    if name == "task":
        edges, labels = [], np.zeros(n, dtype=np.int64)
        for base in range(0, n, 11):
            labels[base: base + 5] = 1
            edges += [(base + a, base + b) for a in range(5) for b in range(a + 1, 5)]
            edges += [(base + a, base + a + 1) for a in range(4, 10)]
            edges.append((base + 10, base + 11) if base + 11 < n else (0, base + 10))
        return np.array(sorted(set(edges)), dtype=np.int32), labels
    if name == "n257d64":                                            # two components: ids 0..99 and 100..256
        parts = [ids[:100], ids[100:]]
    else:
        parts = [ids]
    edges = set()
    for part in parts:
        edges |= {(a, b) for a, b in zip(part[:-1], part[1:])}
        want = len(edges) + chords * len(part) // len(ids)
        while len(edges) < want:
            u, v = sorted(rng.choice(part, 2, replace=False).tolist())
            edges.add((u, v))
    if name == "hub300d8":
        edges |= {(0, v) for v in ids[1:]}
    edges = sorted(edges)
    if name == "multi130d32":                                        # 30 % of the edges listed twice
        twice = rng.random_sample(len(edges)) < 0.3
        edges = sorted(edges + [e for e, t in zip(edges, twice) if t])
    return np.array(edges, dtype=np.int32), None


def run_reference(ref, edges, ids, d, multi):
    """-> (the reference's table in G's node order, its two heat matrices as dense arrays)"""
    import networkx as nx

    G = nx.MultiGraph() if multi else nx.Graph()
    G.add_nodes_from(ids)
    G.add_edges_from(edges.tolist())
    seen = {}
    inner = ref.graphwave_alg

    def alg(*args, **kw):
        out = inner(*args, **kw)
        seen["heat"] = np.stack([out[1][i].toarray() for i in range(2)])
        return out

    ref.graphwave_alg = alg
    try:
        chi = ref.GraphWave(d).train(G)
    finally:
        ref.graphwave_alg = inner
    return np.asarray(chi), seen["heat"]


def longdouble_table(edges, ids, d):
    """the contract's formulas in np.longdouble on the live nodes; taus and time points are the float64 values"""
    from gcc_amd import graphwave as GW

    ld = np.longdouble
    n, T = len(ids), d // 4
    pos = {v: i for i, v in enumerate(ids)}
    a = np.zeros((n, n), dtype=ld)
    for u, v in edges.tolist():
        a[pos[u], pos[v]] += 1
        a[pos[v], pos[u]] += 1
    dinv = 1 / np.sqrt(a.sum(0))
    m = -(dinv[:, None] * a * dinv[None, :])
    order = GW.ORDER
    xx = np.cos((2 * np.arange(1, order + 1, dtype=ld) - 1) / (2 * order) * (4 * np.arctan(ld(1))))
    basis = [np.ones(order, dtype=ld), xx]
    for _ in range(order - 1):
        basis.append(2 * xx * basis[-1] - basis[-2])
    basis = np.vstack(basis)
    heats = []
    for tau in GW.auto_taus(n):
        c = 2 / ld(order) * (np.exp(-ld(tau) * (xx + 1)) * basis).sum(1)
        c[0] /= 2
        x0, x1 = np.eye(n, dtype=ld), m
        h = c[0] * x0 + c[1] * x1
        for k in range(2, order + 1):
            x0, x1 = x1, 2 * (m @ x1) - x0
            h = h + c[k] * x1
        heats.append(np.where(h > ld(GW.THRESHOLD) / n, h, 0))
    sig = np.zeros((n, d), dtype=ld)
    for i, h in enumerate(heats):
        for j, t in enumerate(GW.time_points(d)):
            sig[:, i * 2 * T + 2 * j] = np.cos(ld(t) * h).sum(0) / n
            sig[:, i * 2 * T + 2 * j + 1] = np.sin(ld(t) * h).sum(0) / n
    return sig


def task_margin(table, labels):
    """-> (the smallest fold score, the smallest |decision value| of a held-out row) of the task's classifier on ``table``"""
    from sklearn.linear_model import LogisticRegression
    from sklearn.metrics import f1_score
    from sklearn.multiclass import OneVsRestClassifier

    from gcc_amd.tasks.graph_classification import fold_ids

    y = np.zeros((len(labels), 2), dtype=np.float32)
    y[np.arange(len(labels)), labels] = 1
    fold = fold_ids(y.argmax(axis=1), 0, 10)
    score, margin = 1.0, np.inf
    for f in range(10):
        train, test = fold != f, fold == f
        clf = OneVsRestClassifier(LogisticRegression(C=1000.0, solver="lbfgs")).fit(table[train], y[train])
        pred = np.zeros_like(y[test])
        pred[np.arange(test.sum()), clf.predict_proba(table[test]).argmax(1)] = 1
        score = min(score, f1_score(y[test], pred, average="micro"))
        margin = min(margin, float(np.abs(clf.decision_function(table[test])).min()))
    return score, margin


def make(ref, name):
    from gcc_amd import graphwave as GW
    from tests.graphwave_reference import csr_from_edges

    n_rows, d, chords, keep_heat = FIXTURES[name]
    iso = ISOLATED.get(name, ())
    ids = [i for i in range(n_rows) if i not in iso]
    n = len(ids)
    multi = name == "multi130d32"
    for graph_seed in range(100):
        rng = np.random.RandomState(graph_seed)
        edges, labels = graph(name, n_rows, chords, rng)
        row_ptr, col_idx = csr_from_edges(edges, n_rows)
        live, pre, thr = GW.heat_numpy(row_ptr, col_idx)
        edge_gap = float(np.abs(pre / thr - 1.0).min())
        if edge_gap < EDGE_GAP:
            continue
        nonzero = pre != 0
        gone = nonzero & ~(pre > thr)
        zeroed, zeroed_negative = float(gone.sum() / nonzero.sum()), float((gone & (pre < 0)).sum() / nonzero.sum())
        chi, heat = run_reference(ref, edges, ids, d, multi)
        assert chi.shape == (n, d) and np.array_equal(heat != 0, pre > thr)
        relabel = 0.0
        for _ in range(3):
            perm = rng.permutation(n)                                # node ids[i] is called ids[perm[i]]
            mapped = np.array(ids)[perm]
            lut = {v: int(mapped[i]) for i, v in enumerate(ids)}
            moved = np.array([sorted((lut[u], lut[v])) for u, v in edges.tolist()], dtype=np.int32)
            chi_p, _ = run_reference(ref, moved, ids, d, multi)      # row r: the node called ids[r]
            relabel = max(relabel, float(np.abs(chi_p[perm] - chi).max()))
        longdouble = float(np.abs(longdouble_table(edges, ids, d) - chi).max())
        variant = max(relabel, longdouble)
        restated = GW.embed_numpy(row_ptr, col_idx, d)["chi"][ids]
        extra = {}
        if labels is not None:
            score, margin = task_margin(chi, labels)
            if score < 1.0 or margin < MIN_DECISION:
                raise SystemExit(f"{name}: fold score {score}, smallest decision value {margin}")
            extra.update(labels=labels, margin=margin)
        if keep_heat:
            extra["heat_print"] = heat
        full = np.zeros((n_rows, d))
        full[ids] = chi
        np.savez_compressed(os.path.join(HERE, f"graphwave_{name}.npz"), edges=edges, n_rows=n_rows, d=d, graph_seed=graph_seed, chi=full,
                            variant_distance=variant, relabel_distance=relabel, longdouble_distance=longdouble, edge_gap=edge_gap,
                            zeroed=zeroed, zeroed_negative=zeroed_negative, **extra)
        print(f"{name}: n {n} of {n_rows} d {d} edges {len(edges)} seed {graph_seed} relabel {relabel:.3g} longdouble {longdouble:.3g} "
              f"edge gap {edge_gap:.3g} zeroed {zeroed:.3g} (negative {zeroed_negative:.3g}) restatement {np.abs(restated - chi).max():.3g}")
        return zeroed, zeroed_negative
    raise SystemExit(f"{name}: no candidate graph met the conditions")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    reference = load_reference()
    bites = [make(reference, fixture_name) for fixture_name in (sys.argv[1:] or FIXTURES)]
    if not sys.argv[1:]:
        assert any(z > 0.05 and neg > 0 for z, neg in bites), "the threshold bites in no fixture"
