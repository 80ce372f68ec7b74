"""gcc_graph_tables / gcc_graph_tables_hub_adj (gcc_amd/csrc/graph_tables.hip) against the host's own tables
(gcc_amd.graph.hub_tables, seed_cdf_table), shared by the emulator tier (tests/test_graph_tables_emu.py) and the GPU tier
(tests/test_graph_tables_gpu.py): the same cases and checks; only the library, the pointer function and the device differ.

The integer outputs (summary, hub_index, hub_adj) are compared for exact equality.  The cdf is float64 summed in another order than
NumPy's, so it is pinned by properties, per shard of n_s nodes:
  (a) it never descends;  (b) its last entry is exactly 1.0 and every entry is > 0;  (c) two calls and any grid size give the same
  bits;  (d) max |cdf - exact| <= (n_s + 64) * 2^-53, ``exact`` in np.longdouble from the same degrees -- the a-priori bound of the
  host's sequential cumsum (n_s - 1 roundings), the constant covering the power, the total and the two divisions.
The shapes come from the tiles the library exports (_cabi.GRAPH_TABLES_SCAN_TILE nodes, GRAPH_TABLES_ENTRY_TILE entries).  The
outputs are allocated with guard words on both sides and pre-filled."""
import numpy as np
import pytest
import torch

from gcc_amd import _cabi
from gcc_amd.graph import hub_tables, seed_cdf_table
from gcc_amd.graph_tables import GraphTablesEngine
from gcc_amd.graphgen import check_contract, powerlaw_graph

T, E = _cabi.GRAPH_TABLES_SCAN_TILE, _cabi.GRAPH_TABLES_ENTRY_TILE
GUARD, FILL, G = 0x6B6B6B6B, 0x5A5A5A5A, 8
HUB_DEGREE = 8                                          # small graphs have hubs
HUB_COUNTS = (1, 31, 32, 33, 64, 65)


# ---------------------------------------------------------------- graphs
def csr_of(n, edges):
    """symmetric, loop-free, duplicate-free CSR with sorted rows of the undirected ``edges`` [m, 2]"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    key = np.unique(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]]))
    rows, cols = key // n, key % n
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    rp, ci = rp.astype(np.int32), cols.astype(np.int32)
    check_contract(rp, ci)
    return rp, ci


def ring(n):
    i = np.arange(n)
    return csr_of(n, np.stack([i, (i + 1) % n], axis=1))


def chords(n, seed):
    """a ring with as many random chords: no empty row, mixed degrees"""
    i = np.arange(n)
    rng = np.random.Generator(np.random.PCG64(seed))
    return csr_of(n, np.concatenate([np.stack([i, (i + 1) % n], axis=1), rng.integers(0, n, size=(n, 2))]))


def star(h):
    return csr_of(h + 1, np.stack([np.zeros(h, dtype=np.int64), np.arange(1, h + 1)], axis=1))


def hubs_with_leaves(H, seed, between=True):
    """H hubs with HUB_DEGREE private leaves each (the leaves stand between the hubs in node order), and random hub-hub edges"""
    rng = np.random.Generator(np.random.PCG64(seed))
    block = HUB_DEGREE + 1
    hub = np.arange(H) * block + rng.integers(0, block, size=H)          # the hub's place within its block varies
    edges = []
    for h in range(H):
        leaves = np.setdiff1d(np.arange(h * block, (h + 1) * block), [hub[h]])
        edges.append(np.stack([np.full(len(leaves), hub[h]), leaves], axis=1))
    if between and H > 1:
        edges.append(hub[rng.integers(0, H, size=(3 * H, 2))])
    return csr_of(H * block, np.concatenate(edges))


def union(graphs):
    from gcc_amd.sampler import _disjoint_union

    return _disjoint_union(graphs)


def make_cases():
    """name -> (row_ptr, col_idx, shard_off or None, hub_degree)"""
    c = {}
    c["ring_no_hub"] = (*ring(100), None, HUB_DEGREE)
    for H in HUB_COUNTS:
        c[f"hubs{H}"] = (*hubs_with_leaves(H, H), None, HUB_DEGREE)
    c["hubs_next_to_leaves_only"] = (*hubs_with_leaves(40, 3, between=False), None, HUB_DEGREE)
    c["star_two_entry_tiles"] = (*star(2 * E + 3), None, HUB_DEGREE)
    c["powerlaw"] = (*powerlaw_graph(2000, 12000), None, 16)
    for n in (T - 1, T, T + 1):
        c[f"n{n}"] = (*chords(n, n), None, HUB_DEGREE)
    c["two_nodes"] = (*csr_of(2, [[0, 1]]), None, HUB_DEGREE)
    two = [chords(T + 300, 5), ring(77)]
    c["two_shards"] = (*union(two), np.array([0, T + 300, T + 377]), HUB_DEGREE)
    three = [ring(700), csr_of(2, [[0, 1]]), chords(T + 5, 9)]
    c["three_shards"] = (*union(three), np.array([0, 700, 702, 702 + T + 5]), HUB_DEGREE)
    pl = powerlaw_graph(2000, 12000)
    n = len(pl[0]) - 1                                  # (the generator drops the nodes it left without an edge)
    c["powerlaw_three_shards"] = (*pl, np.array([0, 450, n // 2 + 77, n]), 16)
    return c


CASES = make_cases()
NAMES = list(CASES)
_HOST = {}


def host(name):
    """the host's tables of a case, computed once and handed out read-only"""
    if name not in _HOST:
        rp, ci, so, hd = CASES[name]
        deg = np.diff(rp).astype(np.int64)
        tabs = hub_tables(rp, ci, hd)
        d64 = deg.astype(np.float64)
        ref = dict(summary=np.array([deg.max(), deg.sum(), (deg * deg).sum(), int((deg >= hd).sum())], dtype=np.int64),
                   sb_degree=np.array(float((d64 * d64).sum() / d64.sum())), cdf=seed_cdf_table(rp, so),
                   hub_index=tabs[0] if tabs else None, hub_adj=tabs[1] if tabs else None)
        for v in ref.values():
            if v is not None:
                v.setflags(write=False)
        _HOST[name] = ref
    return _HOST[name]


# ---------------------------------------------------------------- the library under test
class Gt:
    """the library under test, its pointer function and its device (the emulator works on CPU tensors)"""

    def __init__(self, lib, ptr, device):
        self.lib, self.ptr, self.device = lib, ptr, torch.device(device)
        self.engine = GraphTablesEngine(lib, ptr, device)

    def guarded(self, words, dtype=torch.int32):
        """``words`` elements between guards of G elements; 32-bit patterns in every half of a 64-bit element"""
        t = torch.full(((words + 2 * G) * (2 if dtype != torch.int32 else 1),), FILL, dtype=torch.int32, device=self.device)
        k = 2 if dtype != torch.int32 else 1
        t[:G * k] = GUARD
        t[(G + words) * k:] = GUARD
        return t.view(dtype)

    @staticmethod
    def guards_intact(buf, words):
        raw = buf.cpu().view(torch.int32).numpy()
        k = raw.size // (words + 2 * G)
        return (raw[:G * k] == GUARD).all() and (raw[(G + words) * k:] == GUARD).all()

    @staticmethod
    def untouched(buf, words):
        raw = buf.cpu().view(torch.int32).numpy()
        k = raw.size // (words + 2 * G)
        return (raw[G * k:(G + words) * k] == FILL).all()

    def run(self, rp, ci, shard_off=None, hub_degree=HUB_DEGREE, max_hub_bytes=1 << 30, hub_table=True, grid=0):
        """the two bare calls into guarded, pre-filled buffers -> dict(summary int64 [8], cdf, hub_index, hub_adj (None where not
        built), status) as numpy"""
        n, nnz = len(rp) - 1, len(ci)
        rpt = torch.from_numpy(np.ascontiguousarray(rp, dtype=np.int32)).to(self.device)
        cit = torch.from_numpy(np.ascontiguousarray(ci, dtype=np.int32)).to(self.device)
        W = _cabi.GRAPH_TABLES_SUMMARY_WORDS
        summary, cdf, index = self.guarded(W, torch.int64), self.guarded(n, torch.float64), self.guarded(n)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.engine.tables_into(rpt, n, nnz, summary[G:G + W], cdf[G:G + n], index[G:G + n] if hub_table else None, status, shard_off,
                                hub_degree, grid)
        assert self.guards_intact(summary, W) and self.guards_intact(cdf, n) and self.guards_intact(index, n), "a guard word was written"
        if not hub_table:
            assert self.untouched(index, n)
        out = dict(summary=summary[G:G + W].cpu().numpy(), cdf=cdf[G:G + n].cpu().numpy(), hub_index=None, hub_adj=None)
        H = int(out["summary"][3])
        words = (H + 31) // 32
        if hub_table and H > 0 and H * words * 4 <= max_hub_bytes:
            adj = self.guarded(H * words)
            self.engine.hub_adj_into(rpt, cit, n, nnz, index[G:G + n], adj[G:G + H * words], H, words, status, max_hub_bytes, grid)
            assert self.guards_intact(adj, H * words) and self.guards_intact(index, n), "a guard word was written"
            out["hub_index"] = index[G:G + n].cpu().numpy()
            out["hub_adj"] = adj[G:G + H * words].cpu().numpy().view(np.uint32).reshape(H, words)
        out["status"] = int(status.cpu()[0])
        return out


# ---------------------------------------------------------------- checks
def cdf_error(cdf, rp, shard_off=None):
    """properties (a), (b) and (d) of every shard -> the largest |cdf - exact| in units of 2^-53, per shard"""
    deg = np.diff(rp)
    bounds = [0, len(deg)] if shard_off is None or len(shard_off) <= 2 else [int(x) for x in shard_off]
    assert cdf.dtype == np.float64 and len(cdf) == len(deg) and np.isfinite(cdf).all()
    units = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        c = cdf[a:b]
        assert (np.diff(c) >= 0).all(), "(a) the cdf descends"
        assert c[-1] == 1.0 and (c > 0).all(), "(b) the last entry is 1.0, every entry positive"
        w = deg[a:b].astype(np.longdouble) ** np.longdouble(0.75)
        exact = np.cumsum(w) / w.sum()
        err = float(np.abs(c.astype(np.longdouble) - exact).max())
        units.append(err * 2.0 ** 53)
        assert err <= ((b - a) + 64) * 2.0 ** -53, f"(d) {err * 2.0 ** 53:.1f} units of 2^-53 on a shard of {b - a} nodes"
    return units


def check_case(gt, name, grids=(0,), calls=1):
    """every output of a case; ``grids`` / ``calls``: property (c), every run against the first"""
    rp, ci, so, hd = CASES[name]
    ref = host(name)
    first = None
    for grid in grids:
        for _ in range(calls):
            got = gt.run(rp, ci, so, hd, grid=grid)
            assert got["status"] == 0 and np.array_equal(got["summary"][4:], [0, 0, 0, 0])
            # the summary and what DeviceGraph makes of it
            assert np.array_equal(got["summary"][:4], ref["summary"]), (name, got["summary"])
            assert float(got["summary"][2]) / float(got["summary"][1]) == float(ref["sb_degree"])
            # the hub tables: exact
            if ref["hub_index"] is None:
                assert got["hub_index"] is None and got["hub_adj"] is None
            else:
                assert got["hub_index"].dtype == np.int32 and np.array_equal(got["hub_index"], ref["hub_index"]), name
                assert got["hub_adj"].shape == ref["hub_adj"].shape and np.array_equal(got["hub_adj"], ref["hub_adj"]), name
            units = cdf_error(got["cdf"], rp, so)
            print(f"{name} grid {grid}: cdf within {max(units):.2f} units of 2^-53 (host: "
                  f"{max(cdf_error_of_host(name)):.2f})")
            if first is None:
                first = got
            else:
                assert np.array_equal(got["cdf"].view(np.int64), first["cdf"].view(np.int64)), "(c) the cdf's bits changed"
    return first


def cdf_error_of_host(name):
    """the host table's own distance from ``exact``, for the record (no assertion: NumPy's cumsum has its own bound)"""
    rp, _, so, _ = CASES[name]
    deg, cdf = np.diff(rp), host(name)["cdf"]
    bounds = [0, len(deg)] if so is None else [int(x) for x in so]
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        w = deg[a:b].astype(np.longdouble) ** np.longdouble(0.75)
        out.append(float(np.abs(cdf[a:b].astype(np.longdouble) - np.cumsum(w) / w.sum()).max()) * 2.0 ** 53)
    return out


def check_known_values(gt):
    got = gt.run(*CASES["two_nodes"][:3])
    assert np.array_equal(got["cdf"], [0.5, 1.0])
    got = gt.run(*CASES["ring_no_hub"][:3])
    assert np.array_equal(got["summary"][:4], [2, 200, 400, 0]) and got["hub_index"] is None
    assert np.abs(got["cdf"] - np.arange(1, 101) / 100.0).max() <= 164 * 2.0 ** -53
    rp, ci, so, _ = CASES["hubs_next_to_leaves_only"]
    got = gt.run(rp, ci, so)
    assert int(got["summary"][3]) == 40 and got["hub_adj"].shape == (40, 2) and not got["hub_adj"].any()
    assert sorted(got["hub_index"][got["hub_index"] >= 0]) == list(range(40))


def check_hub_table_limits(gt):
    rp, ci, so, hd = CASES["hubs65"]
    ref = host("hubs65")
    need = 65 * 3 * 4
    assert hub_tables(rp, ci, hd, max_bytes=need - 1) is None and hub_tables(rp, ci, hd, max_bytes=need) is not None
    got = gt.run(rp, ci, so, hd, max_hub_bytes=need - 1)
    assert got["hub_index"] is None and got["hub_adj"] is None and int(got["summary"][3]) == 65
    assert np.array_equal(gt.run(rp, ci, so, hd, max_hub_bytes=need)["hub_adj"], ref["hub_adj"])
    got = gt.run(rp, ci, so, hd, hub_table=False)
    assert got["hub_index"] is None and np.array_equal(got["summary"][:4], ref["summary"])
    cdf_error(got["cdf"], rp, so)
    # the engine's own route: one call, the same decisions
    for kw, built in ((dict(), True), (dict(max_hub_bytes=need - 1), False), (dict(hub_table=False), False)):
        t = gt.engine.tables(rp, ci, so, hub_degree=hd, **kw)
        assert (t["hub_adj"] is not None) == built and (t["hub_index"] is not None) == built
        assert [t["max_degree"], t["sum_degree"], t["sum_degree_squared"], t["hubs"]] == list(ref["summary"])
        assert t["sb_degree"] == float(ref["sb_degree"])
        if built:
            assert np.array_equal(t["hub_index"].cpu().numpy(), ref["hub_index"])
            assert np.array_equal(t["hub_adj"].cpu().numpy().view(np.uint32), ref["hub_adj"])
    # the bitmap call refuses what the limit forbids, by name
    with pytest.raises(RuntimeError, match="gcc_graph_tables_hub_adj.*max_hub_bytes"):
        gt.engine.hub_adj_into(torch.zeros(3, dtype=torch.int32, device=gt.device), torch.zeros(2, dtype=torch.int32, device=gt.device), 2, 2,
                               torch.zeros(2, dtype=torch.int32, device=gt.device), torch.zeros(4, dtype=torch.int32, device=gt.device), 2, 1,
                               torch.zeros(1, dtype=torch.int32, device=gt.device), max_hub_bytes=7)


def check_seeds(gt, name):
    """the C oracle draws the same 4,096 seeds from the device's cdf as from the host's"""
    from oracle import sampler as O

    rp, ci, so, hd = CASES[name]
    got = gt.run(rp, ci, so, hd)
    c = O.COracle()
    kw = dict(shard_off=so, batch_size=32) if so is not None else {}
    ours = c.draw_seeds(got["cdf"], 7, 0, 4096, **kw)
    theirs = c.draw_seeds(np.array(host(name)["cdf"]), 7, 0, 4096, **kw)
    assert np.array_equal(ours, theirs)
    if so is not None:                                   # batch i draws from shard i % 3
        which = np.searchsorted(np.asarray(so), ours, side="right") - 1
        assert np.array_equal(which, (np.arange(4096) // 32) % (len(so) - 1))


def check_empty_shard(gt):
    """a shard whose rows are all empty: the bit, the host's message, and 1.0 -- never a NaN"""
    rp, ci = ring(50)
    rp = np.concatenate([rp, np.full(6, rp[-1], dtype=np.int32)])
    so = np.array([0, 50, 56])
    with pytest.raises(ValueError) as err:
        seed_cdf_table(rp, so)
    got = gt.run(rp, ci, so)
    assert got["status"] == _cabi.STATUS_GRAPH_TABLES_EMPTY_SHARD
    assert list(got["summary"][4:6]) == [_cabi.STATUS_GRAPH_TABLES_EMPTY_SHARD, 1]
    assert np.isfinite(got["cdf"]).all() and (got["cdf"][50:] == 1.0).all()
    cdf_error(got["cdf"][:50], rp[:51])
    with pytest.raises(ValueError) as dev:
        gt.engine.tables(rp, ci, so)
    assert str(dev.value) == str(err.value)


def check_refusals(gt):
    dev = gt.device
    n, nnz, W = 5, 8, _cabi.GRAPH_TABLES_SUMMARY_WORDS
    rp = torch.tensor([0, 2, 4, 6, 7, 8], dtype=torch.int32, device=dev)
    ci = torch.zeros(nnz, dtype=torch.int32, device=dev)
    summary, cdf, index, adj = gt.guarded(W, torch.int64), gt.guarded(n, torch.float64), gt.guarded(n), gt.guarded(4)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ok = dict(row_ptr=rp, n=n, nnz=nnz, summary=summary[G:G + W], seed_cdf=cdf[G:G + n], hub_index=index[G:G + n], status=status)
    for member in ("row_ptr", "summary", "seed_cdf"):
        with pytest.raises(RuntimeError, match=f"gcc_graph_tables.*{member} is NULL"):
            gt.engine.tables_into(**{**ok, member: None})
    with pytest.raises(RuntimeError, match="gcc_graph_tables.*shard_off is NULL"):
        gt.engine.tables_into(**ok, num_shards=2)
    with pytest.raises(RuntimeError, match="workspace_bytes 64 is less than gcc_graph_tables_workspace_bytes"):
        gt.engine.tables_into(**ok, workspace_bytes=64)
    for bad in ([1, 3, 5], [0, 3, 4], [0, 3, 3, 5], [0, 4, 3, 5], [0, 6, 5]):
        with pytest.raises(RuntimeError, match="gcc_graph_tables.*shard_off must be increasing node offsets from 0 to n"):
            gt.engine.tables_into(**ok, shard_off=bad)
    for big in (dict(n=2 ** 31), dict(nnz=2 ** 31), dict(n=0)):
        with pytest.raises(RuntimeError, match="must fit int32"):
            a = _cabi.GccGraphTablesArgs(row_ptr=gt.ptr(rp), summary=gt.ptr(ok["summary"]), seed_cdf=gt.ptr(ok["seed_cdf"]),
                                         **{"n": n, "nnz": nnz, **big})
            gt.engine.invoke("gcc_graph_tables", a, gt.engine.workspace(1 << 16, dev), status)
    assert gt.lib.gcc_graph_tables_workspace_bytes(2 ** 31, 1) < 0 and b"must fit int32" in gt.lib.gcc_last_error()
    assert gt.lib.gcc_graph_tables_workspace_bytes(5, 6) < 0 and b"num_shards" in gt.lib.gcc_last_error()
    assert gt.lib.gcc_graph_tables_workspace_bytes(2 ** 31 - 1, 64) > 0
    fill = dict(row_ptr=rp, col_idx=ci, n=n, nnz=nnz, hub_index=index[G:G + n], hub_adj=adj[G:G + 4], num_hubs=4, hub_words=1, status=status)
    for member in ("row_ptr", "col_idx", "hub_index", "hub_adj"):
        with pytest.raises(RuntimeError, match=f"gcc_graph_tables_hub_adj.*{member} is NULL"):
            gt.engine.hub_adj_into(**{**fill, member: None})
    for kw in (dict(num_hubs=0), dict(hub_words=2), dict(num_hubs=6)):
        with pytest.raises(RuntimeError, match="gcc_graph_tables_hub_adj.*num_hubs"):
            gt.engine.hub_adj_into(**{**fill, **kw})
    # nothing was launched
    assert int(status.cpu()[0]) == 0
    for buf, words in ((summary, W), (cdf, n), (index, n), (adj, 4)):
        assert gt.guards_intact(buf, words) and gt.untouched(buf, words)


def check_cpu_tensor_refused(lib):
    eng = GraphTablesEngine(lib, _cabi.dev_ptr, "cpu")
    with pytest.raises(RuntimeError, match="device \\(HIP\\) tensors only"):
        eng.tables(np.array([0, 1, 2]), np.array([1, 0]))
