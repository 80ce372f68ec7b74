"""Generates tests/golden/x2dgl_*.lscc and tests/golden/x2dgl_golden.npz by EXECUTING THE REFERENCE'S OWN
``yuxiao_kdd17_graph_to_dgl`` (gcc/utils/x2dgl.py, loaded from the reference tree; no text of it is copied) on three small files.

DGL does not exist on this stack, so the script puts a minimal stand-in ``dgl`` into ``sys.modules`` at run time: the names the
reference's module imports (``dgl.data.AmazonCoBuy`` / ``Coauthor``, ``dgl.data.utils.save_graphs``: never called here) and a
``DGLGraph`` with the six members the function uses.  Two of them RESTATE DGL's documented behaviour and are not the reference's
own code:

  * ``from_scipy_sparse_matrix(A)`` creates ONE edge per stored non-zero of ``A``, whatever its value (the summed repeats of
    ``tocsr`` become a single edge);
  * ``remove_nodes(ids)`` drops the nodes and their edges and relabels the survivors consecutively IN THEIR OLD ORDER.

Everything else -- which lines are dropped, the two directions, ``coo_matrix(...).tocsr()``, which nodes count as zero-degree and
the four logged numbers -- is the reference's function, executed.  ``in_degrees`` / ``number_of_nodes`` / ``number_of_edges``
count what the stand-in holds; ``readonly`` does nothing.

The files (the reference's text layout: ``<word> n``, n vertex lines, ``<word> m``, m lines ``u v w``):

  x2dgl_small.lscc   9 declared nodes: self loops (one node has nothing else), an edge repeated in both orders, weights other than
                     1, two nodes no line names
  x2dgl_tie.lscc     another graph that keeps as many nodes as x2dgl_small (the CLI's tie rule), repeats only
  x2dgl_hub.lscc     a hub of 70 neighbours (more than a wave's row) written on either side of its lines, a third of them twice,
                     and a sparse rest

Stored per file: n, the lines, the CSR (rows = the stand-in's edges grouped by source and sorted; symmetric, so the in-CSR too)
and ``log``: the four numbers of the reference's own log line (nodes, edges, self loops removed -- two per line --, zero-degree
nodes removed), taken from the log record.

    python tests/golden/make_x2dgl_golden.py
"""
import importlib.util
import logging
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"


class DGLGraph:
    """the stand-in (see the module's docstring)"""

    def __init__(self):
        self.n, self.src, self.dst = 0, np.zeros(0, np.int64), np.zeros(0, np.int64)

    def from_scipy_sparse_matrix(self, a):
        coo = a.tocoo()
        self.n, self.src, self.dst = a.shape[0], coo.row.astype(np.int64), coo.col.astype(np.int64)

    def in_degrees(self):
        import torch

        return torch.from_numpy(np.bincount(self.dst, minlength=self.n))

    def remove_nodes(self, ids):
        ids = np.atleast_1d(np.asarray(ids, dtype=np.int64))
        keep = np.ones(self.n, dtype=bool)
        keep[ids] = False
        new = np.cumsum(keep) - 1
        live = keep[self.src] & keep[self.dst]
        self.src, self.dst, self.n = new[self.src[live]], new[self.dst[live]], int(keep.sum())

    def readonly(self):
        pass

    def number_of_nodes(self):
        return self.n

    def number_of_edges(self):
        return len(self.src)

    def __repr__(self):
        return f"DGLGraph(num_nodes={self.n}, num_edges={len(self.src)})"


def load_reference():
    dgl = types.ModuleType("dgl")
    dgl.DGLGraph = DGLGraph
    data = types.ModuleType("dgl.data")
    data.AmazonCoBuy = data.Coauthor = None
    utils = types.ModuleType("dgl.data.utils")
    utils.save_graphs = None
    dgl.data, data.utils = data, utils
    sys.modules.update({"dgl": dgl, "dgl.data": data, "dgl.data.utils": utils})
    spec = importlib.util.spec_from_file_location("reference_x2dgl", os.path.join(REFERENCE, "gcc", "utils", "x2dgl.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def files():
    """name -> (n, lines [m, 3])"""
    rng = np.random.Generator(np.random.PCG64(2017))
    out = {}
    out["small"] = (9, np.array([[0, 1, 1], [1, 0, 3], [0, 1, 1], [2, 2, 1], [1, 3, 2], [3, 3, 5], [6, 3, 1], [3, 6, 1], [8, 0, 7],
                                 [2, 2, 1], [8, 6, 1]]))                     # 4, 5, 7: never named; 2: loops only
    out["tie"] = (6, np.array([[5, 0, 1], [0, 5, 1], [1, 5, 2], [2, 1, 1], [4, 2, 1], [4, 2, 1], [0, 4, 9]]))   # 3: never named
    hub, leaves = 11, np.delete(np.arange(90), 11)[:70]
    star = np.stack([np.full(70, hub), leaves, rng.integers(1, 9, 70)], axis=1)
    star[::3] = star[::3][:, [1, 0, 2]]
    again = star[1::3][:, [1, 0, 2]]
    rest = np.stack([rng.integers(0, 96, 60), rng.integers(0, 96, 60), np.ones(60, dtype=np.int64)], axis=1)
    out["hub"] = (96, rng.permutation(np.concatenate([star, again, rest, [[40, 40, 1]]]), axis=0))
    return out


def write_lscc(path, n, lines):
    with open(path, "w") as f:
        f.write(f"vertices {n}\n")
        for i in range(n):
            f.write(f"{i} {1000 + 7 * i}\n")
        f.write(f"edges {len(lines)}\n")
        for u, v, w in lines:
            f.write(f"{u} {v} {w}\n")


class Capture(logging.Handler):
    def __init__(self):
        super().__init__()
        self.records = []

    def emit(self, record):
        self.records.append(record)


def main():
    ref = load_reference()
    cap = Capture()
    ref.logger.addHandler(cap)
    out = {}
    for name, (n, lines) in files().items():
        path = os.path.join(HERE, f"x2dgl_{name}.lscc")
        write_lscc(path, n, lines)
        cap.records.clear()
        g = ref.yuxiao_kdd17_graph_to_dgl(path)
        (log,) = [r.args for r in cap.records if "self-loop" in r.msg]
        order = np.lexsort((g.dst, g.src))
        row_ptr = np.zeros(g.n + 1, dtype=np.int64)
        np.cumsum(np.bincount(g.src, minlength=g.n), out=row_ptr[1:])
        out[f"{name}_n"] = np.int64(n)
        out[f"{name}_lines"] = lines.astype(np.int64)
        out[f"{name}_row_ptr"] = row_ptr.astype(np.int32)
        out[f"{name}_col_idx"] = g.dst[order].astype(np.int32)
        out[f"{name}_log"] = np.array(log, dtype=np.int64)
        assert log[0] == g.n and log[1] == len(g.src)
        print(name, "declared", n, "lines", len(lines), "->", log)
    assert out["small_log"][0] == out["tie_log"][0]                 # the tie the CLI's order rule is tested on
    assert np.diff(out["hub_row_ptr"]).max() > 64
    np.savez(os.path.join(HERE, "x2dgl_golden.npz"), **out)


if __name__ == "__main__":
    main()
