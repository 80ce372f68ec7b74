"""gcc_graph_tables / gcc_graph_tables_hub_adj (gcc_amd/csrc/graph_tables.hip) on a real MI355X: the checks of
tests/graph_tables_check.py on every case, each call made twice and at two grid sizes (the bitmap fills in whatever order the
atomics arrive and the cdf must not depend on which workgroup took which tile: only the device can show either),
``DeviceGraph.from_device`` / ``DeviceGraph(tables="device")`` against the host route under the sampler and the C oracle, a corpus of
device pairs in ``LoadBalanceGraphDataset``, and ``train.py --graph-dir``."""
import os

import numpy as np
import pytest
import torch

from tests import graph_tables_check as C

pytestmark = pytest.mark.gpu

RW_HOPS, BATCH, RUN_SEED = 16, 8, 5


@pytest.fixture(scope="module")
def gt():
    from gcc_amd import _cabi

    return C.Gt(_cabi.load(), _cabi.dev_ptr, "cuda:0")


@pytest.mark.parametrize("name", C.NAMES)
def test_tables_are_the_hosts_twice_and_at_two_grid_sizes(gt, name):
    C.check_case(gt, name, grids=(0, 3), calls=2)


def test_known_values(gt):
    C.check_known_values(gt)


def test_no_table_above_the_byte_limit_or_when_not_asked_for(gt):
    C.check_hub_table_limits(gt)


@pytest.mark.parametrize("name", ["powerlaw", "powerlaw_three_shards"])
def test_oracle_draws_the_same_seeds_from_both_cdfs(gt, name):
    C.check_seeds(gt, name)


def test_shard_without_weight_sets_the_bit_and_never_a_nan(gt):
    C.check_empty_shard(gt)


def test_sizes_short_workspace_bad_shards_and_null_members_are_refused_by_name(gt):
    C.check_refusals(gt)


def test_cpu_tensor_is_refused(gt):
    C.check_cpu_tensor_refused(gt.lib)


# ---------------------------------------------------------------- DeviceGraph
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to("cuda:0")


def _hubby():
    """three rows above the sampler's default hub degree, two of them adjacent: the one graph here with hub tables at 512"""
    from gcc_amd.graph import HUB_TABLE_DEGREE

    leaves = HUB_TABLE_DEGREE + 40
    edges = [np.stack([np.full(leaves, h), 3 + h * leaves + np.arange(leaves)], axis=1) for h in range(3)]
    return C.csr_of(3 + 3 * leaves, np.concatenate(edges + [np.array([[0, 2]])]))


def _same_graph(a, b, what):
    for name in ("num_nodes", "num_edges", "max_degree", "sb_degree", "lmax", "num_hubs", "hub_words", "num_shards", "contract_checked",
                 "max_copies", "multigraph", "rw_hops", "restart_prob", "restart_u32"):
        assert getattr(a, name) == getattr(b, name), (what, name, getattr(a, name), getattr(b, name))
    for name in ("row_ptr", "col_idx", "ltab", "hub_index", "hub_adj", "shard_off"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, name)
    for name in ("num_nodes", "num_edges", "ltab_len", "lmax", "num_shards", "flags", "num_hubs", "hub_words", "hub_table_degree"):
        assert getattr(a.c, name) == getattr(b.c, name), (what, "c." + name)


def _first_batch(g):
    from gcc_amd.sampler import DeviceRWRSampler

    s = DeviceRWRSampler(g, batch_size=BATCH, run_seed=RUN_SEED)
    q, k = s.sample(0)
    s.check_status()
    return q.csr_numpy(), k.csr_numpy()


def _same_batches(a, b, what):
    for x, y in zip(a, b):
        assert x["parent_nid"].size > BATCH
        for key in x:
            assert np.array_equal(x[key], y[key]), (what, key)


def _oracle_batch(g, rp, ci, shard_off):
    """the C oracle fed with the graph's own downloaded cdf"""
    from oracle import sampler as O

    c = O.COracle()
    cdf = g.seed_cdf.cpu().numpy()
    seeds = c.draw_seeds(cdf, RUN_SEED, 0, BATCH, shard_off=shard_off, batch_size=BATCH)
    deg = np.diff(rp)
    L = O.max_nodes_table(int(deg.max()), RW_HOPS, 0.8)[deg[seeds]]
    return [c.sample_batch(rp, ci, seeds, L, view, RUN_SEED, 0, O.restart_threshold(0.8)) for view in (0, 1)]


def _three_routes(rp, ci, shard_off, what):
    from gcc_amd.graph import DeviceGraph

    host = DeviceGraph(rp, ci, rw_hops=RW_HOPS, device="cuda:0", validate=True, shard_off=shard_off)
    routes = dict(from_device=DeviceGraph.from_device(_dev(rp), _dev(ci), rw_hops=RW_HOPS, validate="device", shard_off=shard_off),
                  tables_device=DeviceGraph(rp, ci, rw_hops=RW_HOPS, device="cuda:0", validate=True, shard_off=shard_off, tables="device"),
                  tables_device_checked_there=DeviceGraph(rp, ci, rw_hops=RW_HOPS, device="cuda:0", validate="device", shard_off=shard_off,
                                                          tables="device"))
    want = _first_batch(host)
    for name, g in routes.items():
        _same_graph(g, host, (what, name))
        units = C.cdf_error(g.seed_cdf.cpu().numpy(), rp, shard_off)
        print(f"{what} {name}: cdf within {max(units):.2f} units of 2^-53")
        assert g.seed_cdf.dtype == torch.float64 and g.c.seed_cdf == g.seed_cdf.data_ptr()
        _same_batches(_first_batch(g), want, (what, name))
    ref = _oracle_batch(routes["from_device"], rp, ci, shard_off)
    for got, r in zip(_first_batch(routes["from_device"]), ref):
        for key in ("parent_nid", "row_ptr", "col_idx"):
            assert np.array_equal(got[key], r[key]), (what, "oracle", key)
    return host, routes


def test_device_graph_three_routes_on_one_graph():
    rp, ci = C.CASES["powerlaw"][:2]
    _three_routes(rp, ci, None, "powerlaw")


def test_device_graph_three_routes_with_hub_tables():
    rp, ci = _hubby()
    host, routes = _three_routes(rp, ci, None, "hubby")
    assert host.num_hubs == 3 and routes["from_device"].hub_adj is not None
    from gcc_amd.graph import DeviceGraph

    off = DeviceGraph.from_device(_dev(rp), _dev(ci), rw_hops=RW_HOPS, hub_table=False)
    assert off.hub_index is None and off.hub_adj is None and off.num_hubs == 0 and off.c.hub_table_degree == 0
    unchecked = DeviceGraph.from_device(_dev(rp), _dev(ci), rw_hops=RW_HOPS, validate=False)
    assert not unchecked.contract_checked and unchecked.hub_adj is None and unchecked.c.flags == 0
    trusted = DeviceGraph.from_device(_dev(rp), _dev(ci), rw_hops=RW_HOPS, validate=False, trusted=True)
    assert trusted.contract_checked and trusted.num_hubs == 3


@pytest.fixture(scope="module")
def corpus():
    from gcc_amd.graphgen import powerlaw_graph

    return [powerlaw_graph(2500, 15000, 0), powerlaw_graph(1200, 7000, 1), powerlaw_graph(600, 3000, 2)]


@pytest.mark.parametrize("workers", [2, 4])
def test_corpus_of_device_pairs_is_laid_out_like_the_arrays(corpus, workers):
    from gcc_amd.sampler import LoadBalanceGraphDataset

    kw = dict(rw_hops=RW_HOPS, num_workers=workers, num_samples=16, batch_size=BATCH, run_seed=RUN_SEED, device="cuda:0")
    host = LoadBalanceGraphDataset(graph=[(rp.copy(), ci.copy()) for rp, ci in corpus], **kw)
    dev = LoadBalanceGraphDataset(graph=[(_dev(rp), _dev(ci)) for rp, ci in corpus], **kw)
    assert dev.jobs == host.jobs and dev.graph_order == host.graph_order and dev.total == host.total
    assert host.graph.num_shards == min(workers, 3) and dev.graph.contract_checked
    rp, ci = host.graph.row_ptr.cpu().numpy(), host.graph.col_idx.cpu().numpy()
    so = host.graph.shard_off.cpu().numpy()
    host2, routes = _three_routes(rp, ci, so, f"corpus x{workers}")
    _same_graph(dev.graph, host.graph, "dataset")
    C.cdf_error(dev.graph.seed_cdf.cpu().numpy(), rp, so)
    _same_batches(_first_batch(dev.graph), _first_batch(host.graph), "dataset")
    q, k = next(iter(dev))
    hq, hk = next(iter(host))
    _same_batches((q.csr_numpy(), k.csr_numpy()), (hq.csr_numpy(), hk.csr_numpy()), "iteration")


def test_from_device_raises_check_contracts_message():
    from gcc_amd.graph import DeviceGraph
    from gcc_amd.graphgen import check_contract

    rp, ci = C.CASES["powerlaw"][:2]
    row = int(np.argmax(np.diff(rp)))
    short = rp.copy()
    short[row + 1:] -= 1
    lop = np.delete(ci, int(rp[row]))                     # one direction of one edge removed
    with pytest.raises(ValueError) as host:
        check_contract(short, lop)
    with pytest.raises(ValueError) as dev:
        DeviceGraph.from_device(_dev(short), _dev(lop), rw_hops=RW_HOPS, validate="device")
    assert str(dev.value) == str(host.value) and "not symmetric" in str(dev.value)


def test_from_device_refusals_by_name():
    from gcc_amd.graph import DeviceGraph

    rp, ci = C.CASES["powerlaw"][:2]
    with pytest.raises(ValueError, match="a multigraph from device tensors needs validate=\"device\""):
        DeviceGraph.from_device(_dev(rp), _dev(ci), rw_hops=RW_HOPS, validate=False, multigraph=True)
    with pytest.raises(ValueError, match="validate True"):
        DeviceGraph.from_device(_dev(rp), _dev(ci), rw_hops=RW_HOPS, validate=True)
    with pytest.raises(TypeError, match="row_ptr must be a one-dimensional int32 device tensor"):
        DeviceGraph.from_device(rp, _dev(ci), rw_hops=RW_HOPS)
    with pytest.raises(ValueError, match="tables 'gpu'"):
        DeviceGraph(rp, ci, rw_hops=RW_HOPS, device="cuda:0", tables="gpu")
    with pytest.raises(ValueError, match="shard_off must be increasing"):
        DeviceGraph.from_device(_dev(rp), _dev(ci), rw_hops=RW_HOPS, shard_off=[0, 5, 5, len(rp) - 1])


def test_multigraph_from_device_takes_max_copies_from_the_check():
    from gcc_amd.graph import DeviceGraph
    from tests import multigraph_cases as M

    rp, ci = C.CASES["powerlaw"][:2]
    mrp, mci = M.weighted_parent(rp, ci, np.random.RandomState(5))
    host = DeviceGraph(mrp, mci, rw_hops=RW_HOPS, device="cuda:0", validate=True, multigraph=True)
    dev = DeviceGraph.from_device(_dev(mrp), _dev(mci), rw_hops=RW_HOPS, validate="device", multigraph=True)
    assert dev.max_copies == host.max_copies > 1 and not dev.contract_checked and dev.hub_adj is None
    _same_graph(dev, host, "multigraph")
    _same_graph(DeviceGraph(mrp, mci, rw_hops=RW_HOPS, device="cuda:0", validate=True, multigraph=True, tables="device"), host, "multigraph")


# ---------------------------------------------------------------- the entry point
def _write_lscc(path, n, lines):
    with open(path, "w") as f:
        f.write(f"vertices {n}\n")
        f.writelines(f"{i} {1000 + i}\n" for i in range(n))
        f.write(f"edges {len(lines)}\n")
        f.writelines(f"{u} {v} 1\n" for u, v in lines)


def test_train_from_a_folder_of_raw_edge_files(tmp_path, monkeypatch):
    """three .lscc files of random lines with self loops and repeats -> train.py --graph-dir: a finite loss, a checkpoint, and the
    corpus --dgl-file reads from the .bin the converter writes from the same folder"""
    import train
    from gcc_amd import x2dgl
    from gcc_amd.sampler import LoadBalanceGraphDataset

    folder = tmp_path / "raw"
    folder.mkdir()
    names = []
    for i, (n, m) in enumerate(((900, 5000), (1500, 9000), (400, 2500))):
        rng = np.random.Generator(np.random.PCG64(i))
        lines = rng.integers(0, n, size=(m, 2))
        lines = np.concatenate([lines, lines[:50], np.stack([np.arange(20), np.arange(20)], axis=1)])      # repeats, self loops
        names.append(f"g{i}.lscc")
        _write_lscc(folder / names[-1], n, rng.permutation(lines, axis=0))
    made = []

    class Recording(LoadBalanceGraphDataset):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(train, "LoadBalanceGraphDataset", Recording)
    common = ["--exp", "Raw", "--model-path", str(tmp_path / "saved"), "--tb-path", str(tmp_path / "tb"), "--gpu", "0", "--moco",
              "--nce-k", "64", "--batch-size", "16", "--rw-hops", "32", "--num-workers", "2", "--num-copies", "1", "--num-samples", "32", "--epochs", "1",
              "--producer-lanes", "1", "--producer-chunk", "2"]
    args = train.parse_option(common + ["--graph-dir", str(folder), "--graph-files", ",".join(names)])
    args.gpu = args.gpu[0]
    loss = train.main(args)                                 # one epoch of 32 * 2 // 16 = 4 steps
    assert np.isfinite(loss) and os.path.isfile(os.path.join(args.model_folder, "current.pth"))
    ckpt = torch.load(os.path.join(args.model_folder, "current.pth"), map_location="cpu", weights_only=False)
    assert ckpt["opt"].graph_dir == str(folder) and ckpt["opt"].graph_files == ",".join(names) and ckpt["opt"].dgl_file == "./data/small.bin"
    assert "graph" not in os.path.basename(args.model_folder) and not [f for f in os.listdir(folder) if not f.endswith(".lscc")]
    raw = made[0].graph
    # the same folder through the converter and --dgl-file
    x2dgl.main(["--graph-dir", str(folder), "--save-file", str(tmp_path / "corpus.bin"), "--files", ",".join(names)])
    ref = LoadBalanceGraphDataset(rw_hops=32, num_workers=2, num_samples=32, dgl_graphs_file=str(tmp_path / "corpus.bin"), batch_size=16,
                                  device="cuda:0")
    assert made[0].jobs == ref.jobs and made[0].graph_order == ref.graph_order
    for name in ("row_ptr", "col_idx", "shard_off"):
        assert torch.equal(getattr(raw, name), getattr(ref.graph, name)), name
    _same_graph(raw, ref.graph, "train")
