"""Multigraph parents on the wave64 emulator: parallel edges are repeated, adjacent entries of sorted CSR rows.
The dense eigensolver classes count the copies when they assemble D^-1/2 A D^-1/2 (they assigned one coupling per
pair before, silently, with status word 0); the deflation rules hold unchanged; simple graphs keep every bit; the
sampler walks and induces such a parent bit for bit as the C oracle does."""
import os

import numpy as np
import pytest

from gcc_amd.graphgen import check_contract, check_multigraph_contract, powerlaw_graph
from tests import multigraph_cases as C
from tests.hipemu.emu_driver import EmuGraph, emu_sample_batch
from tests.test_posemb_emu import _check, _run, reduced_sizes
from tests.test_sampler_emu import _compare, _dense_graph, _graph_with_super_hub


# ---- eigensolver: one view per dense class and its switch
@pytest.mark.parametrize("n,env", [(40, {}), (40, {"GCC_POSEMB_WAVE": "0"}), (56, {}), (100, {"GCC_POSEMB_PAIR": "1"}), (100, {"GCC_POSEMB_PAIR": "0"}),
                                   (200, {"GCC_POSEMB_CHEB": "0"}), (200, {"GCC_POSEMB_CHEB": "1"}),
                                   (420, {"GCC_POSEMB_CHEB": "0"})])
def test_dense_classes_count_parallel_edges(n, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    view = C.eig_view(n)
    lo, hi = C.EIG_CASES[n][1]
    assert lo <= reduced_sizes(view)[0] <= hi
    assert C.float64_gap(view) > 1e-3                 # the wanted subspace is unique: _check compares the Gram matrices
    x, evals, raw = _run(view)
    assert _run.arnoldi_steps == 0 and _run.status[3] == 0
    assert (_run.status[1] >= 2) == (env.get("GCC_POSEMB_CHEB") == "1")     # filter rounds: the sparse block class ran
    _check(view, x, evals, raw)


def test_deflation_rules_under_multiplicity():
    """Twin leaves on a hub with tripled edges, stalks with single hub edges, a look-alike stalk whose hub edge is doubled,
    nodes tied to their only neighbour by two edges, spiders with k = n - 2: a twin leaf is a row of ONE entry, a stalk's
    middle node a row of two DIFFERENT columns one of which is such a leaf."""
    view = C.deflation_view()
    red = reduced_sizes(view)
    sizes = np.diff(view["node_off"].numpy())
    # what the rules must (and must not) collapse: 4 twins -> 1; 3 stalks -> 1 (the look-alike and the doubled pendants
    # stay); 3 stalks -> 1; 3 stalks -> 1 (the doubled leg stays); 5 twins -> 1 and 4 stalks -> 1
    assert (sizes - red).tolist() == [3, 4, 4, 4, 4 + 6]
    assert 64 < red[4] <= 128
    x, evals, raw = _run(view)
    assert _run.arnoldi_steps == 0 and _run.status[3] == 0
    _check(view, x, evals, raw)


def test_simple_graphs_keep_every_bit(monkeypatch):
    """A run of one entry writes the float it wrote before the assembly counted copies: pos, evals and raw of simple graphs
    in every dense class (and the block class) are the bits recorded at the commit before (make_posemb_simple_golden.py)."""
    from tests.golden.make_posemb_simple_golden import SWITCHES, views

    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "posemb_simple_bits.npz"))
    for name, view in views().items():
        for key, arr in zip(("pos", "evals", "raw"), _run(view)):
            assert np.array_equal(np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32), z["%s_%s" % (name, key)]), (name, key)


# ---- parent-graph contract
def test_multigraph_contract():
    rp, ci = powerlaw_graph(300, 1500, 3)
    check_multigraph_contract(rp, ci)                                     # a simple graph is a multigraph
    mrp, mci = C.weighted_parent(rp, ci, np.random.RandomState(0))
    check_multigraph_contract(mrp, mci)
    with pytest.raises(ValueError, match="duplicate"):
        check_contract(mrp, mci)
    distinct = np.array([len(np.unique(mci[a:b])) for a, b in zip(mrp[:-1], mrp[1:])])
    row = int(np.flatnonzero(distinct >= 2)[0])                           # a row that holds two or more distinct columns
    bad = mci.copy()                                                      # unsorted row
    bad[mrp[row]:mrp[row + 1]] = bad[mrp[row]:mrp[row + 1]][::-1]
    with pytest.raises(ValueError, match="sorted"):
        check_multigraph_contract(mrp, bad)
    # one copy more in one direction only
    e = int(mrp[row])
    rp2 = mrp.copy()
    rp2[row + 1:] += 1
    with pytest.raises(ValueError, match="equal copy counts"):
        check_multigraph_contract(rp2, np.insert(mci, e, mci[e]))
    loop = np.insert(mci, e, row)                                         # a self loop (kept sorted)
    order = np.argsort(loop[rp2[row]:rp2[row + 1]], kind="stable")
    loop[rp2[row]:rp2[row + 1]] = loop[rp2[row]:rp2[row + 1]][order]
    with pytest.raises(ValueError, match="self loop"):
        check_multigraph_contract(rp2, loop)
    with pytest.raises(ValueError, match="zero-degree"):
        check_multigraph_contract(np.r_[mrp, mrp[-1]].astype(np.int32), mci)


# ---- sampler: bit-exact against the C oracle on the expanded CSR, contract unchecked
def _multi_parent(rp, ci, seed):
    mrp, mci = C.weighted_parent(rp, ci, np.random.RandomState(seed))
    assert len(mci) > len(ci)
    return mrp, mci


def test_sampler_walks_and_induces_the_multigraph(coracle):
    rp, ci = _multi_parent(*powerlaw_graph(800, 4000, 3), seed=1)
    g = EmuGraph(rp, ci, rw_hops=32, contract_checked=False)
    res = _compare(coracle, rp, ci, g, 6, 7, 0, seeds=np.array([0, 5, 17, 100, 333, len(rp) - 2], np.int32))
    col, rptr = res[0]["col_idx"], res[0]["row_ptr"]
    inner = np.ones(len(col), bool)
    inner[rptr[:-1][rptr[:-1] < len(col)]] = False
    assert (np.diff(col)[inner[1:]] == 0).any()                           # the induced rows carry parallel edges
    _compare(coracle, rp, ci, g, 5, 11, 40)                               # drawn seeds: ~ (multigraph degree)^0.75


def test_sampler_big_walk_class_on_a_multigraph(coracle):
    rp0, ci0, hub = _graph_with_super_hub()
    rp, ci = _multi_parent(rp0, ci0, seed=2)
    g = EmuGraph(rp, ci, rw_hops=64, contract_checked=False)
    assert g.ltab[np.diff(rp)[hub]] > 1024
    nb = ci0[rp0[hub]:rp0[hub] + 2]
    _compare(coracle, rp, ci, g, 3, 5, 0, seeds=np.array([hub, nb[0], nb[1]], np.int32))


@pytest.mark.parametrize("budget", [900, 2000])
def test_sampler_big_induce_class_on_a_multigraph(coracle, budget):
    """A trace budget (``ltab``) of 900 on this 400-node parent collects 260..305 members per subgraph, whatever the seeds:
    it runs the small induce class with long multigraph rows.  2000 collects 333..347, the class over 320 members."""
    rp, ci = _multi_parent(*_dense_graph(400, 0.6, 2), seed=3)
    g = EmuGraph(rp, ci, rw_hops=64, ltab=np.full(int(np.diff(rp).max()) + 1, budget, dtype=np.int32), contract_checked=False)
    res = _compare(coracle, rp, ci, g, 2, 3, 0)
    sizes = np.diff(res[0]["node_off"])
    assert (sizes.min() > 320) == (budget == 2000)
    assert np.diff(res[0]["row_ptr"]).max() > sizes.max() - 1             # an induced row longer than n - 1


def test_sampler_multigraph_overflow_is_flagged_not_truncated():
    """An induced multigraph row can hold more than n - 1 entries: an edge capacity sized for simple subgraphs
    (n (n - 1) per subgraph) overflows and must say so."""
    rp, ci = _multi_parent(*_dense_graph(120, 0.9, 4), seed=4)
    L = 100
    g = EmuGraph(rp, ci, rw_hops=64, ltab=np.full(int(np.diff(rp).max()) + 1, L, dtype=np.int32), contract_checked=False)
    B = 2
    res, status, _ = emu_sample_batch(g, B, 3, 0, edge_cap=8 * B * (L + 1) ** 2)
    assert status == 0
    n = np.diff(res[0]["node_off"])
    assert int(res[0]["edge_off"][-1]) > int((n * (n - 1)).sum())         # more entries than any simple subgraph has
    _, status, _ = emu_sample_batch(g, B, 3, 0, edge_cap=int((n * (n - 1)).sum()))
    assert status & 4


# ---- eval encoders on repeated entries: the oracle run on the same CSR
def test_fused_eval_and_chain_on_repeated_entries():
    from tests.wide_edges_check import EMU

    C.check_fused_eval_and_chain(EMU, rtol=1e-4, atol=2e-5)


def test_any_width_chain_on_repeated_entries():
    from tests.wide_edges_check import EMU

    C.check_any_width_chain(EMU, rtol=1e-4, atol=2e-5)


def test_resident_embed_on_repeated_entries():
    from tests.wide_edges_check import EMU

    C.check_resident_embed(EMU)


def test_gat_forward_on_repeated_entries():
    from tests.wide_edges_check import EMU

    C.check_gat_forward(EMU, rtol=1e-4, atol=2e-5)


def test_whole_path_on_a_weighted_coauthor_network(tmp_path):
    from tests.wide_edges_check import EMU

    C.check_whole_path(EMU, tmp_path, rtol=1e-4, atol=2e-5)
