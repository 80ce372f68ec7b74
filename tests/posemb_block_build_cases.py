"""Synthetic items for the sparse block class's matrix build, Cholesky and expansion (posemb_cheb_kernel), shared by
tests/test_posemb_block_build_emu.py, tests/test_posemb_block_build_gpu.py and the recorder of their fixtures
(tests/golden/make_posemb_block_build_golden.py).  Every builder is deterministic.

The matrix build hands rows of at most 64 entries to groups of 8 lanes (128 rows per pass of a 1,024-thread workgroup,
8 entries per round) and longer rows to whole waves; the Cholesky factorisation runs on 32 columns at a time, a 64-column
block replaying the first half's steps on the second; the expansion puts two nodes on a wave, one per half.  The cases
are the smallest that cross each of those boundaries."""
import numpy as np
import torch

from tests import multigraph_cases as C

ROW_LENGTHS = (1, 7, 8, 9, 16, 17, 63, 64, 65)         # kept entries of the rows case (b) places
CSR_CAP = 12288                                         # kChCsrCap: directed edges of a deflated item the block class holds


def _view(n, edges):
    import scipy.sparse as sp

    e = np.array(sorted(set((min(i, j), max(i, j)) for i, j in edges)))
    a = sp.csr_matrix((np.ones(2 * len(e)), (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=(n, n))
    a.sort_indices()
    return dict(node_off=torch.tensor([0, n]), row_ptr=torch.from_numpy(a.indptr.astype(np.int64)),
                col_idx=torch.from_numpy(a.indices.astype(np.int64)))


def kept_rows(view):
    """-> (kept flag per node, kept entries per node) of a one-item SIMPLE view by the deflation rules of
    gcc_amd/csrc/posemb.hip: of t >= 2 leaves of one parent the first stays, of s >= 2 pendant two-paths of one hub the
    first (middle node and leaf)."""
    rp, ci = view["row_ptr"].numpy(), view["col_idx"].numpy()
    n = len(rp) - 1
    deg = np.diff(rp)
    keep = np.ones(n, bool)
    leaf = deg == 1
    par = np.where(leaf, ci[np.minimum(rp[:-1], len(ci) - 1)], -1)
    for p in np.unique(par[leaf]):
        ls = np.flatnonzero(par == p)
        if len(ls) >= 2:
            keep[ls[1:]] = False
    hub = np.full(n, -1)
    for a in np.flatnonzero(deg == 2):
        x, y = ci[rp[a]], ci[rp[a] + 1]
        if leaf[x] != leaf[y]:
            hub[a] = y if leaf[x] else x
    for h in np.unique(hub[hub >= 0]):
        mids = np.flatnonzero(hub == h)
        if len(mids) >= 2:
            for a in mids[1:]:
                x, y = ci[rp[a]], ci[rp[a] + 1]
                keep[a] = False
                keep[x if leaf[x] else y] = False
    cnt = np.array([int(keep[ci[rp[i]:rp[i + 1]]].sum()) if keep[i] else 0 for i in range(n)])
    return keep, cnt


def sparse_item(n, seed):
    """(a) nothing to deflate, ~6 entries per row: n' = n"""
    return C.view_of(*_csr(C.sparse_power_graph(n, np.random.RandomState(seed))))


def _csr(a):
    return a.indptr.astype(np.int32), a.indices.astype(np.int32)


def row_length_item():
    """(b) ~140 kept rows.  Rows with ROW_LENGTHS kept entries stand at the first and last slot of a lane group's pass and in
    its middle, once bare and once with three twin leaves and two pendant two-paths attached, whose ids are spread over the
    id range: the long rows then hold dropped entries between kept ones inside one 8-entry round, and the rows of 63 / 64 /
    65 kept entries are longer than a wave with the attachments."""
    rng = np.random.RandomState(2)
    core = 112                                          # ids 0, 3, 6, ... (every third id): the attachments fall in between
    ids = 3 * np.arange(core)
    spare = [i for i in range(3 * core + 60) if i % 3 or i >= 3 * core]
    rng.shuffle(spare)
    edges = [(ids[i], ids[i + 1]) for i in range(core - 1)]
    edges += [(ids[i], ids[j]) for i in range(core) for j in range(i + 2, core) if rng.rand() < 0.02]
    special = []
    for length in ROW_LENGTHS:
        for attach in (False, True):
            v = spare.pop()
            reps = 2 if attach else 0                   # a twin group and a stalk group leave one kept entry each
            if length - reps <= 0:
                continue
            nb = rng.choice(ids, size=length - reps, replace=False)
            edges += [(v, int(u)) for u in nb]
            if attach:
                for _ in range(3):
                    edges.append((v, spare.pop()))
                for _ in range(2):
                    a, b = spare.pop(), spare.pop()
                    edges += [(v, a), (a, b)]
            special.append((v, length, attach))
    used = sorted(set(i for e in edges for i in e))
    relabel = {u: r for r, u in enumerate(used)}        # order-preserving: the interleaving of the ids survives
    view = _view(len(used), [(relabel[i], relabel[j]) for i, j in edges])
    return view, [(relabel[v], length, attach) for v, length, attach in special]


def stalky_item(stalks, seed=11):
    """(c) a 150-node core with ``stalks`` pendant two-paths on node 0: the quotient has to deliver 32 - (stalks - 1) pairs"""
    from tests.test_posemb_emu import _stalky

    n, edges = _stalky(np.random.RandomState(seed), 150, 0.03, [(0, stalks)])
    return _view(n, edges)


def multigraph_item():
    """(d) 200 rows, every undirected edge 1, 1, 2, 3 or 7 times: doubled, tripled and longer runs of adjacent entries"""
    return C.eig_view(200)


def dense_item(n=200, p=0.36, seed=5):
    """(e) more than CSR_CAP kept directed edges in ~200 rows: the block class hands it to the dense classes"""
    rng = np.random.RandomState(seed)
    edges = [(i, i + 1) for i in range(n - 1)] + [(i, j) for i in range(n) for j in range(i + 2, n) if rng.rand() < p]
    return _view(n, edges)


def batch(views):
    """one view holding the items of ``views`` in order"""
    no, rp, ci = [0], [0], []
    for v in views:
        o, e = no[-1], rp[-1]
        vn, vr, vc = (v[k].numpy() for k in ("node_off", "row_ptr", "col_idx"))
        assert len(vn) == 2
        no.append(o + int(vn[1]))
        rp += list(e + vr[1:])
        ci += list(o + vc)
    return dict(node_off=torch.tensor(no), row_ptr=torch.tensor(rp, dtype=torch.int64), col_idx=torch.tensor(ci, dtype=torch.int64))


def cases():
    """name -> (view, hidden, items the block class hands on)"""
    b_view, _ = row_length_item()
    return {
        "sizes": (batch([sparse_item(129, 1), sparse_item(131, 2)]), 32, 0),
        "rows": (b_view, 32, 0),
        "narrow": (stalky_item(25), 32, 0),            # 24 stalk contrasts: at most 8 pairs wanted -> the 32-column block
        "wide": (stalky_item(4), 32, 0),               # 3 contrasts: 29 pairs wanted -> the 64-column block, half-1 replay
        "multigraph": (multigraph_item(), 32, 0),
        "dense": (dense_item(), 32, 1),
        "k16": (sparse_item(131, 2), 16, 0),           # 16 live lanes per half-wave
    }


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32)
