"""Positional embedding kernels (gcc_amd/csrc/posemb.hip) on the wave64 emulator vs dense
float64 eigendecompositions.  Eigenvectors are only defined up to sign / rotation inside
degenerate eigenspaces (and the reference seeds ARPACK randomly, data_util.py:248), so parity is
asserted on invariants: eigenvalues, residuals, orthonormality, unit rows, and -- whenever the
wanted invariant subspace is unique -- the Gram matrix x x^T of the normalised rows."""
import numpy as np
import pytest
import torch

from gcc_amd.graphgen import powerlaw_graph, tiny_graphs
from gcc_amd.posemb import DevicePosEmb
from oracle import posemb as P
from oracle import sampler as O
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_encoder import CpuBatch

HID = 32


def _run(view, hid=None):
    hid = HID if hid is None else hid            # (read at call time: a caller may have set HID)
    b = CpuBatch(dict(view, pos_undirected=torch.zeros(int(view["node_off"][-1]), hid)))
    pe = DevicePosEmb(b.batch_size, b.parent_nid.numel(), hid, device="cpu", lib=emu_lib(),
                      ptr=lambda t: 0 if t is None else t.data_ptr())
    evals = torch.zeros(b.batch_size, hid)
    raw = torch.zeros(b.parent_nid.numel(), hid)
    pe(b, evals=evals, raw=raw)
    assert int(pe.status[0]) == 0
    _run.arnoldi_steps = int(pe.status[2])
    _run.status = [int(v) for v in pe.status]
    return b.pos_undirected.numpy(), evals.numpy(), raw.numpy()


_DENSE = {}


def _dense_eigh(M):
    """np.linalg.eigh(M) in float64, computed once per matrix and shared read-only by every check that asks for it"""
    import hashlib

    key = (M.shape[0], hashlib.sha1(np.ascontiguousarray(M).tobytes()).digest())
    if key not in _DENSE:
        s, u = np.linalg.eigh(M)
        s.setflags(write=False)
        u.setflags(write=False)
        _DENSE[key] = (s, u)
    return _DENSE[key]


def _check(view, x, evals, raw, tol=2e-4, hid=None):
    """-> the items whose Gram matrix was compared (the wanted subspace is unique there)"""
    hid = HID if hid is None else hid            # (read at call time: a caller may have set HID)
    no = view["node_off"].numpy()
    rp, ci = view["row_ptr"].numpy(), view["col_idx"].numpy()
    gram = []
    for b in range(len(no) - 1):
        lo, hi = no[b], no[b + 1]
        n = hi - lo
        k = min(n - 2, hid)
        xb, ub = x[lo:hi], raw[lo:hi]
        if k <= 0:
            assert not xb.any()
            continue
        M = P.normalized_adjacency(rp[lo:hi + 1] - rp[lo], ci[rp[lo]:rp[hi]] - lo).toarray()
        s, u = _dense_eigh(M)
        assert np.allclose(evals[b, :k], s[-k:], atol=tol), (b, n)            # eigsh(which="LA"): ascending top-k
        assert not evals[b, k:].any() and not xb[:, k:].any()                   # F.pad(..., hidden - k)
        U = ub[:, :k].astype(np.float64)
        assert np.abs(U.T @ U - np.eye(k)).max() < tol                          # orthonormal eigenvectors
        assert np.abs(M @ U - U * evals[b, :k]).max() < tol                     # residual
        norms = np.linalg.norm(xb[:, :k], axis=1)
        assert np.all((np.abs(norms - 1) < 1e-4) | (norms == 0))               # sklearn normalize(norm="l2")
        gap_ok = n - k - 1 < 0 or s[-k] - s[-k - 1] > 1e-3                      # wanted subspace unique?
        if gap_ok:
            ud = u[:, -k:]
            nd = np.linalg.norm(ud, axis=1, keepdims=True)
            # (a float64 row below 1e-9 is a zero row -- an isolated node next to non-zero eigenvalues -- and not the unit row
            #  that normalising its rounding noise would make: the device row must then be zero too)
            xd = np.where(nd < 1e-9, 0.0, ud / np.maximum(nd, 1e-300))
            assert np.abs(xb @ xb.T - xd @ xd.T).max() < 5e-3, (b, n)          # same rows up to a rotation
            # the reference's own solver (ARPACK, random start): single-vector Krylov may miss copies of a repeated
            # eigenvalue (seen at n = 101 on the 1M-node graph), so it is only compared where it found the dense answer itself
            xr, _ = P.eigen_decomposition(n, k, __import__("scipy.sparse").sparse.csr_matrix(M), hid,
                                          rng=np.random.RandomState(b))
            if np.abs(xr @ xr.T - xd @ xd.T).max() < 1e-6:
                assert np.abs(xb @ xb.T - xr @ xr.T).max() < 5e-3, (b, n)
            gram.append(b)
    return gram


DIRECT_MAX = 704          # GCC_POSEMB_BIG_MAX: the direct solver's last size class
SLOT_MAX = 384            # GCC_POSEMB_DIRECT_MAX: 128 KiB-of-LDS workspace class


def reduced_sizes(view, stalks=True):
    """Deflated size n' of every subgraph: t >= 2 leaves of one parent count once, and (``stalks``) s >= 2 pendant
    two-paths hub - a - leaf of one hub count as one."""
    no = view["node_off"].numpy()
    rp, ci = view["row_ptr"].numpy(), view["col_idx"].numpy()
    out = []
    for b in range(len(no) - 1):
        lo, hi = no[b], no[b + 1]
        deg = np.diff(rp[lo:hi + 1])
        leaves = np.where(deg == 1)[0]
        cnt = np.bincount(ci[rp[lo + leaves]] - lo, minlength=hi - lo) if len(leaves) else np.zeros(hi - lo, int)
        size = int(hi - lo) - int(np.maximum(cnt - 1, 0).sum())
        if stalks:
            hubs = []
            for a in np.where(deg == 2)[0]:
                x, y = ci[rp[lo + a]] - lo, ci[rp[lo + a] + 1] - lo
                if (deg[x] == 1) != (deg[y] == 1):
                    hubs.append(y if deg[x] == 1 else x)
            if hubs:
                size -= 2 * int(np.maximum(np.bincount(hubs) - 1, 0).sum())
        out.append(size)
    return np.array(out)


def _sub(view, b):
    no = view["node_off"].numpy()
    lo, hi = int(no[b]), int(no[b + 1])
    return lo, hi, dict(node_off=torch.tensor([0, hi - lo]), row_ptr=view["row_ptr"][lo:hi + 1] - view["row_ptr"][lo],
                        col_idx=view["col_idx"][view["row_ptr"][lo]:view["row_ptr"][hi]] - lo)


def check_by_path(view, x, evals, raw, only=None, hid=None, gram=None):
    """STRICT invariants where the direct solver ran (deflated size <= DIRECT_MAX), Krylov invariants elsewhere.
    ``gram``: a list that collects the items whose Gram matrix was compared."""
    red = reduced_sizes(view)
    for b in (range(len(red)) if only is None else only):
        lo, hi, sub = _sub(view, b)
        if red[b] <= DIRECT_MAX and hi - lo <= 1024:
            done = _check(sub, x[lo:hi], evals[b:b + 1], raw[lo:hi], hid=hid)
            if gram is not None and done:
                gram.append(int(b))
        else:
            _check_krylov(sub, x[lo:hi], evals[b:b + 1], raw[lo:hi], hid=hid)
    return red


def _sampled_views(rw_hops, B, run_seed):
    rp, ci = powerlaw_graph(3000, 30000, 3)
    c = O.COracle()
    seeds = c.draw_seeds(O.seed_cdf(rp), run_seed, 0, B)
    L = O.max_nodes_table(int(np.diff(rp).max()), rw_hops, 0.8)[np.diff(rp)[seeds]]
    r = c.sample_batch(rp, ci, seeds, L, 0, run_seed, 0, O.restart_threshold(0.8))
    return dict(node_off=torch.from_numpy(r["node_off"].astype(np.int64)),
                row_ptr=torch.from_numpy(r["row_ptr"].astype(np.int64)),
                col_idx=torch.from_numpy(r["col_idx"].astype(np.int64)))


def test_sampled_subgraphs_lds_direct_path():
    view = _sampled_views(rw_hops=48, B=6, run_seed=4)
    assert np.diff(view["node_off"].numpy()).max() <= 128
    _check(view, *_run(view))


def test_tiny_and_degenerate_graphs():
    # n = 1, 2 (k <= 0 -> zeros), path, star (null space of dimension n - 2), complete graph (n-1 fold eigenvalue)
    blocks = [(1, []), (2, [(0, 1)]), (3, [(0, 1), (1, 2)])]
    for name in ("path5", "star6", "k4", "tri_tail"):
        rp, ci = tiny_graphs()[name]
        n = len(rp) - 1
        blocks.append((n, [(i, int(j)) for i in range(n) for j in ci[rp[i]:rp[i + 1]] if i < j]))
    blocks.append((40, [(0, i) for i in range(1, 40)]))
    import scipy.sparse as sp
    node_off, rows, cols = [0], [], []
    for n, edges in blocks:
        o = node_off[-1]
        for i, j in edges:
            rows += [o + i, o + j]
            cols += [o + j, o + i]
        node_off.append(o + n)
    N = node_off[-1]
    a = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(N, N))
    a.sort_indices()
    view = dict(node_off=torch.tensor(node_off), row_ptr=torch.from_numpy(a.indptr.astype(np.int64)),
                col_idx=torch.from_numpy(a.indices.astype(np.int64)))
    _check(view, *_run(view))


def _check_krylov(view, x, evals, raw, tol=1e-3, hid=None):
    """Large subgraphs go through the single-vector Krylov-Schur path: like ARPACK it may miss extra
    copies of an exactly repeated eigenvalue, so eigenvalues are checked as 'true eigenvalues, top of
    the spectrum, every distinct wanted eigenvalue present'."""
    hid = HID if hid is None else hid            # (read at call time: a caller may have set HID)
    no = view["node_off"].numpy()
    rp, ci = view["row_ptr"].numpy(), view["col_idx"].numpy()
    for b in range(len(no) - 1):
        lo, hi = no[b], no[b + 1]
        n = hi - lo
        if n <= 128:
            continue
        k = hid
        M = P.normalized_adjacency(rp[lo:hi + 1] - rp[lo], ci[rp[lo]:rp[hi]] - lo).toarray()
        s = _dense_eigh(M)[0]
        got = evals[b]
        assert np.all(np.diff(got) >= -1e-6)                                     # ascending
        assert np.abs(got[:, None] - s[None, :]).min(axis=1).max() < tol         # each one is an eigenvalue
        wanted = s[s >= got[0] + 10 * tol]                                       # every eigenvalue above the cut
        assert np.abs(wanted[:, None] - got[None, :]).min(axis=1).max() < tol    # ... is represented
        assert abs(got[-1] - 1.0) < tol                                          # connected ego-net: lambda_max = 1
        U = raw[lo:hi, :k].astype(np.float64)
        assert np.abs(U.T @ U - np.eye(k)).max() < tol
        assert np.abs(M @ U - U * got).max() < tol
        norms = np.linalg.norm(x[lo:hi, :k], axis=1)
        isolated = np.diff(rp[lo:hi + 1]) == 0                                   # (no existing caller has one: unit rows throughout)
        assert np.all((np.abs(norms - 1) < 1e-4) | (isolated & (norms == 0)))


@pytest.mark.parametrize("cheb", ["0", "1"])
def test_large_subgraphs_workspace_resident_direct_path(cheb, monkeypatch):
    """128 < n' <= 384.  cheb=0: the dense workspace class (the matrix lives in a workspace slot, everything else as in
    the LDS classes); cheb=1 (the default): the sparse Chebyshev class takes them first.  Either way the STRICT
    invariants hold (all multiplicities) and no Krylov iteration runs."""
    monkeypatch.setenv("GCC_POSEMB_CHEB", cheb)
    rp, ci = powerlaw_graph(20000, 400000, 1)
    c = O.COracle()
    deg = np.diff(rp)
    hubs = np.argsort(deg)[-2:].astype(np.int32)
    L = np.array([300, 420], dtype=np.int32)
    r = c.sample_batch(rp, ci, hubs, L, 0, 3, 0, O.restart_threshold(0.6))
    sizes = np.diff(r["node_off"])
    assert sizes.min() > 128
    view = dict(node_off=torch.from_numpy(r["node_off"].astype(np.int64)),
                row_ptr=torch.from_numpy(r["row_ptr"].astype(np.int64)),
                col_idx=torch.from_numpy(r["col_idx"].astype(np.int64)))
    red = reduced_sizes(view)
    assert ((red > 128) & (red <= SLOT_MAX)).all(), red
    x, evals, raw = _run(view)
    assert _run.arnoldi_steps == 0
    _check(view, x, evals, raw)


def skewed_dense_graph(n, seed=1):
    """A connected graph of n nodes with skewed degrees, like an ego-net, and no twin leaves -> scipy CSR"""
    import scipy.sparse as sp

    rng = np.random.RandomState(seed)
    w = 1.0 / np.arange(1, n + 1) ** 0.5                        # skewed degrees, like an ego-net
    pr = np.minimum(1.0, 6.0 * np.outer(w, w) / w.mean())
    up = np.triu(rng.rand(n, n) < pr, 1)
    up[np.arange(n - 1), np.arange(1, n)] = True                # connected
    a = sp.csr_matrix((up | up.T).astype(np.float64))
    a.sort_indices()
    deg = np.diff(a.indptr)
    assert (deg >= 2).all() or np.bincount(a.indices[a.indptr[:-1][deg == 1]]).max() < 2
    return a


@pytest.mark.parametrize("cheb", ["0", "1"])
def test_krylov_fallback_above_the_direct_limit(cheb, monkeypatch):
    """Deflated size > 704 (no twin leaves at all).  cheb=0: thick-restart Krylov-Schur (single vector, ARPACK-like
    invariants); cheb=1: the sparse block class is tried first and hands this (dense) graph on."""
    monkeypatch.setenv("GCC_POSEMB_CHEB", cheb)
    n = 760
    a = skewed_dense_graph(n)
    view = dict(node_off=torch.tensor([0, n]), row_ptr=torch.from_numpy(a.indptr.astype(np.int64)),
                col_idx=torch.from_numpy(a.indices.astype(np.int64)))
    x, evals, raw = _run(view)
    # 30k undirected edges do not fit the block class's LDS edge list (12288 directed): with cheb=1 the item is handed
    # on (status[3] counts it) and, being larger than the dense classes too, ends in the Krylov class either way
    assert _run.arnoldi_steps > 0 and _run.status[3] == (1 if cheb == "1" else 0)
    _check_krylov(view, x, evals, raw)


def _view_of(n, edges):
    import scipy.sparse as sp

    e = np.array(edges)
    a = sp.csr_matrix((np.ones(2 * len(e)), (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=(n, n))
    a.sum_duplicates()
    a.data[:] = 1
    a.sort_indices()
    return dict(node_off=torch.tensor([0, n]), row_ptr=torch.from_numpy(a.indptr.astype(np.int64)),
                col_idx=torch.from_numpy(a.indices.astype(np.int64)))


@pytest.mark.parametrize("cheb,stalks", [("0", "0"), ("1", "0"), ("1", "1")])
def test_hub_ego_net_with_repeated_eigenvalues(cheb, stalks, monkeypatch):
    """The shape of a hub seed's ego-net at rw_hops 256 on the 1M-node graph (n ~ 850): a hub with hundreds of pendant
    two-paths (hub - a_i - leaf_i), which puts 1/sqrt(2) into the spectrum hundreds of times.  Exact multiplicities are
    out of reach of a single-vector Krylov iteration (ARPACK returns other, smaller eigenvalues for the copies it cannot
    see).  stalks=1 (the default): the stalks are deflated exactly, 63 quotient nodes remain and the copies are contrast
    vectors.  stalks=0 (twin leaves only, deflated ~ 480): cheb=1 the block Chebyshev class (whatever a block holds of a
    repeated eigenvalue's eigenspace are eigenvectors); cheb=0: 384 < n' <= 704 by the dense direct solver.  STRICT
    invariants in every case."""
    monkeypatch.setenv("GCC_POSEMB_CHEB", cheb)
    monkeypatch.setenv("GCC_POSEMB_STALKS", stalks)
    rng = np.random.RandomState(3)
    t = 210
    edges = [(0, 1 + i) for i in range(t)] + [(1 + i, 1 + t + i) for i in range(t)]
    core0 = 1 + 2 * t
    core = 60
    edges += [(0, core0 + i) for i in range(core)]
    edges += [(core0 + i, core0 + j) for i in range(core) for j in range(i + 1, core) if rng.rand() < 0.1]
    n = core0 + core
    view = _view_of(n, edges)
    red = reduced_sizes(view, stalks=stalks == "1")
    if stalks == "1":
        assert red[0] == 63
    else:
        assert SLOT_MAX < red[0] <= DIRECT_MAX, red
    x, evals, raw = _run(view)
    assert _run.arnoldi_steps == 0 and _run.status[3] == 0
    assert (_run.status[1] >= 2) == (cheb == "1" and stalks == "0")    # filter rounds of the block class
    assert np.sum(np.abs(evals[0] - 2 ** -0.5) < 1e-4) >= 25          # the repeated eigenvalue fills the top 32
    _check(view, x, evals, raw)


def _stalky(rng, core, p, hubs, n_twins=()):
    """A random connected core plus, per (hub, s) in ``hubs``, s pendant two-paths and, per (parent, t) in ``n_twins``,
    t leaves."""
    edges = [(i, j) for i in range(core) for j in range(i + 1, core) if rng.rand() < p]
    edges += [(i, i + 1) for i in range(core - 1)]
    nxt = core
    for hub, s_ in hubs:
        for _ in range(s_):
            edges += [(hub, nxt), (nxt, nxt + 1)]
            nxt += 2
    for par, t in n_twins:
        edges += [(par, nxt + i) for i in range(t)]
        nxt += t
    return nxt, edges


def stalky_view():
    """Graphs with pendant two-paths for every solver class: stalk groups on several hubs (sizes 2..40), twin leaves on the
    same hubs, top-k cuts inside the 1/sqrt(2) cluster, and tiny graphs whose k = n - 2 reaches the null space and the
    -1/sqrt(2) copies.  -> (view, deflated sizes with stalks, with twin leaves only)"""
    import scipy.sparse as sp

    rng = np.random.RandomState(11)
    blocks = []
    blocks.append((7, [(0, 1), (1, 2), (0, 3), (3, 4), (0, 5), (5, 6)]))                   # spider: 3 stalks, k = 5
    blocks.append(_stalky(rng, 1, 0.0, [(0, 3)], [(0, 2)]))                                # 3 stalks + 2 twin leaves on one node
    blocks.append(_stalky(rng, 2, 1.0, [(0, 2), (1, 4)], [(1, 3)]))
    blocks.append(_stalky(rng, 30, 0.15, [(0, 12), (3, 2), (7, 5)], [(0, 6), (9, 2)]))     # wave / small class
    blocks.append(_stalky(rng, 60, 0.08, [(0, 40), (1, 17), (2, 9)], [(0, 30), (5, 4)]))   # n' ~ 70 after, ~190 before: mid class
    blocks.append(_stalky(rng, 150, 0.03, [(0, 25), (10, 3), (20, 14)], [(4, 9)]))         # n' ~ 160: sparse block class
    node_off, rows, cols = [0], [], []
    for n, edges in blocks:
        o = node_off[-1]
        for i, j in set((min(i, j), max(i, j)) for i, j in edges):
            rows += [o + i, o + j]
            cols += [o + j, o + i]
        node_off.append(o + n)
    N = node_off[-1]
    a = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(N, N))
    a.sort_indices()
    view = dict(node_off=torch.tensor(node_off), row_ptr=torch.from_numpy(a.indptr.astype(np.int64)),
                col_idx=torch.from_numpy(a.indices.astype(np.int64)))
    red, red0 = reduced_sizes(view), reduced_sizes(view, stalks=False)
    assert (red0 - red >= 2).all() and 64 < red[4] <= 128 < red0[4] and red[5] > 128, (red, red0)
    return view, red, red0


@pytest.mark.parametrize("wave", ["0", "1"])
def test_stalk_deflation_in_every_solver_class(wave, monkeypatch):
    """Pendant two-paths are deflated exactly in the one-wave teams, the block classes and the sparse block class
    (stalky_view); STRICT invariants."""
    monkeypatch.setenv("GCC_POSEMB_WAVE", wave)
    view, red, red0 = stalky_view()
    x, evals, raw = _run(view)
    assert _run.arnoldi_steps == 0 and _run.status[3] == 0 and _run.status[1] >= 2, _run.status
    assert np.sum(np.abs(evals[4] - 2 ** -0.5) < 1e-5) >= 20
    _check(view, x, evals, raw)


def test_sparse_graph_beyond_the_dense_classes_is_solved_by_the_block_class():
    """n' = 900 > GCC_POSEMB_BIG_MAX, no twin leaves, ~6 edges per node: only the sparse Chebyshev block class (up to
    1024 nodes) and the Krylov class reach this size; the block class runs (status[1] = its filter rounds, no Arnoldi
    steps, nothing handed on) and the STRICT invariants hold."""
    import scipy.sparse as sp

    rng = np.random.RandomState(7)
    n = 900
    w = 1.0 / np.arange(1, n + 1) ** 0.6
    pr = np.minimum(1.0, 3.0 * np.outer(w, w) / (w.mean() ** 2 * n))
    up = np.triu(rng.rand(n, n) < pr, 1)
    up[np.arange(n - 1), np.arange(1, n)] = True
    a = sp.csr_matrix((up | up.T).astype(np.float64))
    a.sort_indices()
    deg = np.diff(a.indptr)
    assert a.nnz < 12000 and ((deg >= 2).all() or np.bincount(a.indices[a.indptr[:-1][deg == 1]]).max() < 2)
    view = dict(node_off=torch.tensor([0, n]), row_ptr=torch.from_numpy(a.indptr.astype(np.int64)),
                col_idx=torch.from_numpy(a.indices.astype(np.int64)))
    assert reduced_sizes(view)[0] > DIRECT_MAX
    x, evals, raw = _run(view)
    assert _run.arnoldi_steps == 0 and _run.status[1] >= 2 and _run.status[3] == 0, _run.status
    _check(view, x, evals, raw)


def test_leafy_large_subgraph_is_solved_exactly_by_deflation():
    """n = 331 original nodes, but 290 of them are leaves of 3 hubs: the deflated problem has ~45 nodes and
    goes through the dense direct solver, so the STRICT invariants (all multiplicities) must hold."""
    import scipy.sparse as sp

    rng = np.random.RandomState(0)
    core = 40
    edges = [(i, j) for i in range(core) for j in range(i + 1, core) if rng.rand() < 0.15]
    edges += [(i, i + 1) for i in range(core - 1)]                 # connected
    nxt = core
    for hub, t in ((0, 200), (5, 80), (9, 10), (12, 1)):
        edges += [(hub, nxt + i) for i in range(t)]
        nxt += t
    n = nxt
    e = np.array(edges)
    a = sp.csr_matrix((np.ones(2 * len(e)), (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=(n, n))
    a.sum_duplicates()
    a.data[:] = 1
    a.sort_indices()
    view = dict(node_off=torch.tensor([0, n]), row_ptr=torch.from_numpy(a.indptr.astype(np.int64)),
                col_idx=torch.from_numpy(a.indices.astype(np.int64)))
    assert n > 128
    _check(view, *_run(view))


@pytest.mark.parametrize("pair", ["1", "0"])
def test_both_size_classes_of_the_direct_solver(pair, monkeypatch):
    """Deflated sizes on both sides of 64: the one-wave teams and the 65..128 class -- four-wave teams with the matrix rows in registers
    (the default) or, GCC_POSEMB_PAIR=0, the 1,024-thread LDS instantiation of posemb_direct_kernel.  Both meet the strict invariants;
    their eigenvalues agree to fp32 accuracy."""
    monkeypatch.setenv("GCC_POSEMB_PAIR", pair)
    view = _sampled_views(rw_hops=160, B=10, run_seed=11)
    red = reduced_sizes(view)
    assert (red <= 64).any() and ((red > 64) & (red <= 128)).any(), red
    x, evals, raw = _run(view)
    check_by_path(view, x, evals, raw)
    keep = test_both_size_classes_of_the_direct_solver.__dict__.setdefault("evals", {})
    keep[pair] = evals.copy()
    if len(keep) == 2:
        assert np.abs(keep["1"] - keep["0"]).max() < 5e-6


def test_multi_view_call_matches_per_view_invariants():
    """gcc_posemb_multi: three views (different sizes, all four solver classes' lists shared) in one launch set."""
    views = [_sampled_views(rw_hops=48, B=4, run_seed=s) for s in (21, 22, 23)]
    batches = [CpuBatch(dict(v, pos_undirected=torch.zeros(int(v["node_off"][-1]), HID))) for v in views]
    cap = max(b.parent_nid.numel() for b in batches)
    pe = DevicePosEmb(4, cap, HID, device="cpu", lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr(),
                      max_views=3, num_buffers=2)
    pe.multi(batches)
    assert int(pe.status[0]) == 0
    single = DevicePosEmb(4, cap, HID, device="cpu", lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr())
    for v, b in zip(views, batches):
        n = int(v["node_off"][-1])
        x = b.pos_undirected[:n].numpy().copy()
        ref = CpuBatch(dict(v, pos_undirected=torch.zeros(n, HID)))
        ev, raw = torch.zeros(4, HID), torch.zeros(cap, HID)
        single(ref, evals=ev, raw=raw)
        xs = ref.pos_undirected[:n].numpy()
        no = v["node_off"].numpy()
        for i in range(4):                                   # same rows up to sign / rotation inside eigenspaces
            lo, hi = no[i], no[i + 1]
            assert np.abs(x[lo:hi] @ x[lo:hi].T - xs[lo:hi] @ xs[lo:hi].T).max() < 5e-3
        _check(v, xs, ev.numpy(), raw[:n].numpy())


def test_subgraph_larger_than_its_share_of_node_cap_is_refused_loudly():
    """The Krylov class sizes its vectors as node_cap / batch_size: a large subgraph beyond that gets zeros and status
    bit 16, and check_status() raises (never a silent wrong answer or an out-of-bounds access)."""
    import scipy.sparse as sp

    rng = np.random.RandomState(5)
    n = 1100                                                  # more nodes than any block / dense class takes -> Krylov class
    up = np.triu(rng.rand(n, n) < 0.02, 1)
    up[np.arange(n - 1), np.arange(1, n)] = True
    a = sp.csr_matrix((up | up.T).astype(np.float64))
    a.sort_indices()
    small = sp.csr_matrix(np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], dtype=np.float64))
    blk = sp.block_diag([a, small, small, small], format="csr")
    blk.sort_indices()
    view = dict(node_off=torch.tensor([0, n, n + 3, n + 6, n + 9]), row_ptr=torch.from_numpy(blk.indptr.astype(np.int64)),
                col_idx=torch.from_numpy(blk.indices.astype(np.int64)))
    b = CpuBatch(dict(view, pos_undirected=torch.ones(n + 9, HID)), node_cap=n + 9)
    pe = DevicePosEmb(4, n + 9, HID, device="cpu", lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr())
    pe(b)
    assert int(pe.status[0]) & 16
    assert not b.pos_undirected[:n].any()                    # zeros, not garbage
    with pytest.raises(RuntimeError):
        pe.check_status()


def dense_views():
    """Dense ego-nets next to sparse ones of the same size: a 60-node random graph of density 0.7 (one-wave team, ~2500 CSR
    entries), a 110-node one of density 0.8 (65..128 class, ~9600 entries) and two sparse ones.  (Written for an experiment
    that staged the ego-net's CSR in LDS -- these do not fit such a staging area -- and kept as coverage of rows much longer
    than a wave: no deflation applies, every row is a hub's.)"""
    rng = np.random.default_rng(3)
    views = []
    for n, p in ((60, 0.7), (60, 0.06), (110, 0.8), (110, 0.04)):
        edges = [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < p]
        edges += [(i, i + 1) for i in range(n - 1)]                       # connected
        views.append(_view_of(n, edges))
    return views


def test_dense_ego_nets_without_anything_to_deflate():
    for view in dense_views():
        x, evals, raw = _run(view)
        _check(view, x, evals, raw)


def test_workspace_sizes_are_the_recorded_ones(monkeypatch):
    """Callers cache gcc_posemb_multi_workspace_bytes: the sizes recorded before the workspace got its one layout
    (tests/golden/make_posemb_workspace_golden.py, default grid caps) are the sizes it returns."""
    import json
    import os

    monkeypatch.delenv("GCC_POSEMB_GRID_CAPS", raising=False)
    monkeypatch.delenv("GCC_POSEMB_GATED_CAPS", raising=False)
    rows = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "posemb_workspace_bytes.json")))
    assert [(r["views"], r["batch_size"], r["node_cap"]) for r in rows] == [
        (1, 6, 6 * 257), (1, 8, 8 * 1025), (3, 4, 4 * 257), (16, 256, 256 * 257)]
    lib = emu_lib()
    for r in rows:
        assert lib.gcc_posemb_multi_workspace_bytes(r["views"], r["batch_size"], r["node_cap"], HID) == r["bytes"], r


GUARD = 4096


def guarded_workspace(pe, device):
    """Puts ``pe``'s workspace into a 256-byte-aligned slice of exactly the advertised size inside a buffer filled with
    0xA5, at least GUARD bytes of it on either side -> a function that asserts both bands are still intact."""
    buf = torch.full((pe.nbytes + 2 * GUARD + 256,), 0xA5, dtype=torch.uint8, device=device)
    off = GUARD + (-(buf.data_ptr() + GUARD)) % 256
    pe.workspace = buf[off:off + pe.nbytes]
    assert pe.workspace.data_ptr() % 256 == 0 and pe.workspace.numel() == pe.nbytes

    def intact():
        assert bool((buf[:off] == 0xA5).all()), "write in front of the workspace"
        assert bool((buf[off + pe.nbytes:] == 0xA5).all()), "write past the advertised workspace size"
    return intact


def big_and_krylov_view():
    """Two dense graphs without twin leaves: deflated size 400 (with GCC_POSEMB_CHEB=0 the 385..704 class) and 760 (Krylov)."""
    import scipy.sparse as sp

    a = sp.block_diag([skewed_dense_graph(400, seed=2), skewed_dense_graph(760)], format="csr")
    a.sort_indices()
    view = dict(node_off=torch.tensor([0, 400, 1160]), row_ptr=torch.from_numpy(a.indptr.astype(np.int64)),
                col_idx=torch.from_numpy(a.indices.astype(np.int64)))
    red = reduced_sizes(view)
    assert SLOT_MAX < red[0] <= DIRECT_MAX < red[1], red
    return view


@pytest.mark.parametrize("case,cheb", [("stalky", "1"), ("stalky", "0"), ("big+krylov", "0")])
def test_writes_stay_inside_the_advertised_workspace(case, cheb, monkeypatch):
    """Every solver class carves its slots, tables and buffers out of the one workspace layout: a call touches nothing
    outside the size gcc_posemb_multi_workspace_bytes advertised.  stalky_view() reaches the one-wave teams, the four-wave
    65..128 class, the block class and (cheb=0) the 129..384 slot class; the third case the 385..704 class and Krylov
    (the emulator's slowest kind of item: its restarts on 760 nodes are most of this case's ~14 s)."""
    monkeypatch.setenv("GCC_POSEMB_CHEB", cheb)
    view = stalky_view()[0] if case == "stalky" else big_and_krylov_view()
    sizes = np.diff(view["node_off"].numpy())
    b = CpuBatch(dict(view, pos_undirected=torch.zeros(int(view["node_off"][-1]), HID)),
                 node_cap=len(sizes) * (int(sizes.max()) + 1))      # the Krylov class sizes its vectors as node_cap / batch_size
    pe = DevicePosEmb(b.batch_size, b.parent_nid.numel(), HID, device="cpu", lib=emu_lib(),
                      ptr=lambda t: 0 if t is None else t.data_ptr())
    intact = guarded_workspace(pe, "cpu")
    evals = torch.zeros(b.batch_size, HID)
    raw = torch.zeros(b.parent_nid.numel(), HID)
    pe(b, evals=evals, raw=raw)
    intact()
    assert int(pe.status[0]) == 0
    n = int(view["node_off"][-1])
    x = b.pos_undirected[:n].numpy()
    if case == "stalky":
        assert int(pe.status[2]) == 0
        _check(view, x, evals.numpy(), raw[:n].numpy())
    else:
        assert int(pe.status[2]) > 0                                           # Arnoldi steps: the Krylov class ran
        check_by_path(view, x, evals.numpy(), raw[:n].numpy())
