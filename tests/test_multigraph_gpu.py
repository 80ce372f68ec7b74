"""Multigraph parents on a real MI355X (the emulator twins are in tests/test_multigraph_emu.py): the dense eigensolver
classes count parallel edges, the deflation rules hold under multiplicity, and the device sampler walks and induces a
multigraph parent bit for bit as the C oracle does."""
import numpy as np
import pytest
import torch

from tests import multigraph_cases as C
from tests.test_posemb_emu import HID, _check, reduced_sizes

pytestmark = pytest.mark.gpu


def _batch_of(view):
    from gcc_amd.sampler import BatchedCSR

    no, rp, ci = (view[k].numpy() for k in ("node_off", "row_ptr", "col_idx"))
    B, n = len(no) - 1, int(no[-1])
    q = BatchedCSR(B, torch.from_numpy(no.astype(np.int32)).cuda(), torch.from_numpy(rp[no].astype(np.int32)).cuda(),
                   torch.zeros(n, dtype=torch.int32, device="cuda"),
                   torch.from_numpy(np.repeat(np.arange(B), np.diff(no)).astype(np.int32)).cuda(),
                   torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(ci.astype(np.int32)).cuda())
    q.pos_undirected = torch.zeros(n, HID, device="cuda")
    return q, B, n


def _device_posemb(view):
    from gcc_amd.posemb import DevicePosEmb

    q, B, n = _batch_of(view)
    pe = DevicePosEmb(B, n, HID, device="cuda", seed=7)
    evals = torch.zeros(B, HID, device="cuda")
    raw = torch.zeros(n, HID, device="cuda")
    pe(q, evals=evals, raw=raw)
    pe.check_status(strict=True)
    status = [int(v) for v in pe.status.cpu().tolist()]
    return q.pos_undirected[:n].cpu().numpy(), evals.cpu().numpy(), raw[:n].cpu().numpy(), status


@pytest.mark.parametrize("n,env", [(40, {}), (40, {"GCC_POSEMB_WAVE": "0"}), (56, {}), (100, {"GCC_POSEMB_PAIR": "1"}), (100, {"GCC_POSEMB_PAIR": "0"}),
                                   (200, {"GCC_POSEMB_CHEB": "0"}), (200, {"GCC_POSEMB_CHEB": "1"}),
                                   (420, {"GCC_POSEMB_CHEB": "0"})])
def test_dense_classes_count_parallel_edges_on_device(n, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    view = C.eig_view(n)
    lo, hi = C.EIG_CASES[n][1]
    assert lo <= reduced_sizes(view)[0] <= hi
    assert C.float64_gap(view) > 1e-3                 # the wanted subspace is unique: _check compares the Gram matrices
    x, evals, raw, status = _device_posemb(view)
    assert status[2] == 0 and status[3] == 0
    assert (status[1] >= 2) == (env.get("GCC_POSEMB_CHEB") == "1")
    _check(view, x, evals, raw)


def test_deflation_rules_under_multiplicity_on_device():
    view = C.deflation_view()
    x, evals, raw, status = _device_posemb(view)
    assert status[2] == 0 and status[3] == 0
    _check(view, x, evals, raw)


def _device_sample(rp, ci, B, run_seed, rw_hops, seeds=None, ltab=None):
    from gcc_amd.graph import DeviceGraph
    from gcc_amd.sampler import DeviceRWRSampler
    from oracle import sampler as O

    g = DeviceGraph(rp, ci, rw_hops=rw_hops, ltab=ltab, multigraph=True)
    assert not g.contract_checked and g.c.flags == 0 and g.hub_index is None and g.max_copies > 1
    s = DeviceRWRSampler(g, B, run_seed=run_seed)
    views = s.sample(0, seeds=None if seeds is None else torch.from_numpy(np.asarray(seeds, np.int32)).cuda())
    s.check_status()
    c = O.COracle()
    used = s.last_seeds().cpu().numpy()
    oseeds = c.draw_seeds(O.seed_cdf(rp), run_seed, 0, B) if seeds is None else np.asarray(seeds, np.int32)
    assert used.tolist() == oseeds.tolist()
    L = g.ltab.cpu().numpy()[np.diff(rp)[oseeds]]
    out = []
    for view, gb in enumerate(views):
        ref = c.sample_batch(rp, ci, oseeds, L, view, run_seed, 0, g.restart_u32)
        got = gb.csr_numpy()
        for key in ("node_off", "parent_nid", "row_ptr", "col_idx"):
            assert np.array_equal(got[key], ref[key]), (view, key)
        out.append(got)
    return out


def test_sampler_walks_and_induces_the_multigraph_on_device():
    from gcc_amd.graphgen import powerlaw_graph

    rp, ci = C.weighted_parent(*powerlaw_graph(800, 4000, 3), np.random.RandomState(1))
    got = _device_sample(rp, ci, 6, 7, 32, seeds=[0, 5, 17, 100, 333, len(rp) - 2])
    col, rptr = got[0]["col_idx"], got[0]["row_ptr"]
    inner = np.ones(len(col), bool)
    inner[rptr[:-1][rptr[:-1] < len(col)]] = False
    assert (np.diff(col)[inner[1:]] == 0).any()                           # the induced rows carry parallel edges


@pytest.mark.parametrize("budget", [900, 2000])
def test_sampler_big_induce_class_on_a_multigraph_on_device(budget):
    """(budget 900 stays under 320 members on this parent, 2000 passes them: tests/test_multigraph_emu.py)"""
    from tests.test_sampler_emu import _dense_graph

    rp, ci = C.weighted_parent(*_dense_graph(400, 0.6, 2), np.random.RandomState(3))
    got = _device_sample(rp, ci, 2, 3, 64, ltab=np.full(int(np.diff(rp).max()) + 1, budget, dtype=np.int32))
    sizes = np.diff(got[0]["node_off"])
    assert (sizes.min() > 320) == (budget == 2000)
    assert np.diff(got[0]["row_ptr"]).max() > sizes.max() - 1             # an induced row longer than n - 1


# ---- eval encoders on repeated entries: the oracle run on the same CSR (rtol 1e-3, atol 1e-4 on the device)
def test_fused_eval_and_chain_on_repeated_entries_on_device():
    from tests.wide_edges_check import GPU

    C.check_fused_eval_and_chain(GPU, rtol=1e-3, atol=1e-4)


def test_any_width_chain_on_repeated_entries_on_device():
    from tests.wide_edges_check import GPU

    C.check_any_width_chain(GPU, rtol=1e-3, atol=1e-4)


def test_resident_embed_on_repeated_entries_on_device():
    from tests.wide_edges_check import GPU

    C.check_resident_embed(GPU)


def test_gat_forward_on_repeated_entries_on_device():
    from tests.wide_edges_check import GPU

    C.check_gat_forward(GPU, rtol=1e-3, atol=1e-4)


def test_whole_path_on_a_weighted_coauthor_network_on_device(tmp_path):
    from tests.wide_edges_check import GPU

    C.check_whole_path(GPU, tmp_path, rtol=1e-3, atol=1e-4)
