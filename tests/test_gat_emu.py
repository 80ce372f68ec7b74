"""The GAT kernels (csrc/gat.hip) on the CPU emulator build against the float64 restatement: forward output and every
parameter gradient, at the defaults and at edges (empty / one-node graphs, an isolated node, a long hub row,
edge multiplicity 2, a batch below the buffers' capacity, norm off, a second configuration)."""
import pytest
import torch

from gcc_amd.encoder import GatEngine, gat_params
from tests.gat_check import gat_encoder, kernel_grads, reference, symmetric_batch, worst_rel
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_encoder import CpuBatch


def _engine():
    return GatEngine(lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr())


def _check(enc, batch, mult=1, cap_extra=37, tol=2e-4):
    g = CpuBatch(batch, node_cap=int(batch["node_off"][-1]) + cap_extra)
    g.edge_multiplicity = mult
    B = g.batch_size
    dout = torch.randn(B, enc.output_dim, generator=torch.Generator().manual_seed(5))
    out, grads, _ = kernel_grads(enc, _engine(), g, dout)
    ref_out, ref_grads = reference(enc, batch, dout, mult=mult)
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out.double(), ref_out, rtol=tol, atol=tol)
    for k in ref_grads:
        assert torch.isfinite(grads[k]).all(), k
    worst, name = worst_rel(grads, ref_grads)
    assert worst < tol, (worst, name)
    return grads


def test_defaults_against_float64():
    enc = gat_encoder()
    _check(enc, symmetric_batch([7, 12, 1, 5], seed=1))


def test_second_config_and_norm_off():
    enc = gat_encoder(hidden=32, heads=2, layers=2, T=2, Lr=1, norm=False, pos=8, deg_emb=8, max_degree=16)
    _check(enc, symmetric_batch([9, 4, 6], pos_dim=8, seed=2))


def test_edges_empty_graph_isolated_node_hub_row():
    enc = gat_encoder(hidden=48, heads=4, layers=3, T=3, Lr=2, pos=16, deg_emb=8, max_degree=8)
    # graph 1 empty (a padding graph), graph 2 one node, node 3 isolated, graph 3 a hub row of 70 entries
    batch = symmetric_batch([6, 0, 1, 90], pos_dim=16, p=0.02, seed=3, isolated=(3,), extra_star=(3, 70))
    _check(enc, batch, cap_extra=300)


def test_edge_multiplicity_two():
    enc = gat_encoder(hidden=32, heads=4, layers=2, T=2, Lr=2, pos=8, deg_emb=8, max_degree=6)
    _check(enc, symmetric_batch([8, 10], pos_dim=8, p=0.5, seed=4), mult=2)


def test_gradients_are_bit_identical_across_calls():
    enc = gat_encoder(hidden=32, heads=2, layers=2, T=2, Lr=1, pos=8, deg_emb=8, max_degree=16)
    batch = symmetric_batch([9, 4, 6], pos_dim=8, seed=6)
    g = CpuBatch(batch)
    dout = torch.randn(3, 32)
    _, g1, _ = kernel_grads(enc, _engine(), g, dout)
    _, g2, _ = kernel_grads(enc, _engine(), g, dout)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_backward_accumulates():
    enc = gat_encoder(hidden=16, heads=2, layers=1, T=1, Lr=1, pos=4, deg_emb=4, max_degree=8)
    batch = symmetric_batch([5, 3], pos_dim=4, seed=7)
    g = CpuBatch(batch)
    eng = _engine()
    dout = torch.randn(2, 16)
    out, saved, p, w = eng.forward(enc, g)
    t1 = [torch.zeros_like(t) for _, _, t in gat_params(enc)]
    eng.backward(enc, p, w, dout, t1)
    t2 = [x.clone() for x in t1]
    eng.backward(enc, p, w, dout, t2, accumulate=True)
    for a, b in zip(t1, t2):
        torch.testing.assert_close(b, 2 * a)


@pytest.mark.parametrize("bad", [dict(hidden=96, heads=4), dict(hidden=64, heads=3)])
def test_gat_refuses_unsupported_widths(bad):
    with pytest.raises(NotImplementedError, match="up to 64"):
        gat_encoder(**bad)


def test_degree_embedding_size_zero_is_refused_at_construction():
    """the kernels read a degree embedding; a model without one used to fail at its first forward ("a weight pointer is NULL")"""
    with pytest.raises(NotImplementedError, match="degree_embedding_size"):
        gat_encoder(deg_emb=0)


def test_mpnn_is_refused_with_the_supported_list():
    from gcc_amd.encoder import GraphEncoder

    with pytest.raises(NotImplementedError, match="gat"):
        GraphEncoder(gnn_model="mpnn", degree_input=True)
