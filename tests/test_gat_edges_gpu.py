"""The GAT kernels (csrc/gat.hip) on a real MI355X at their shape edges: the case table of tests/gat_check.py
(EDGE_CASES, the one tests/test_gat_edges_emu.py runs on the emulator) against the float64 restatement, two passes pending
through GraphEncoder.forward, and bit-identical gradients at heads 3.  The emulator is lock-step: a missing barrier or a
cross-wave LDS reuse at these shapes can only show here.  Every batch is small: the file needs seconds of GPU time."""
import pytest
import torch

from tests.gat_check import (CASE_IDS, EDGE_CASES, DeviceBatch, case_inputs, dress_batch, gat_encoder, kernel_grads,
                             reference_of, symmetric_batch, worst_rel_shared)
from tests.gat_reference import forward_of, params_of

pytestmark = pytest.mark.gpu
OUT_TOL, GRAD_TOL = 1e-4, 1e-3        # tests/test_gat_gpu.py::test_small_hand_built_batch_on_device's


def _run(case):
    from gcc_amd.encoder import GatEngine

    enc, batch, dout, kw = case_inputs(case)
    g = dress_batch(DeviceBatch(batch, cap_extra=case["cap_extra"]), case)
    enc = enc.cuda()
    out, grads, _ = kernel_grads(enc, GatEngine(), g, dout.cuda())
    torch.cuda.synchronize()
    return enc, batch, dout, kw, out, grads


@pytest.mark.parametrize("case", EDGE_CASES, ids=CASE_IDS)
def test_case_against_float64_on_device(case):
    enc, batch, dout, kw, out, grads = _run(case)
    ref_out, ref_grads = reference_of(enc, batch, dout, kw)
    assert torch.isfinite(out).all()
    for k in ref_grads:
        assert torch.isfinite(grads[k]).all(), k
    out_err = float((out.double().cpu() - ref_out).abs().max())
    worst, name = worst_rel_shared(grads, ref_grads)
    print(f"{case['name']}: out err {out_err:.2e}; worst gradient entry / scale {worst:.2e} ({name})")
    torch.testing.assert_close(out.double().cpu(), ref_out, rtol=OUT_TOL, atol=OUT_TOL)
    assert worst < GRAD_TOL, (worst, name)


def test_heads3_gradients_are_bit_identical_across_calls():
    """no float atomics, and no race between the S = 64 / 3 edge slots of a wave or between workgroups"""
    case = next(c for c in EDGE_CASES if c["name"] == "h48_heads3_hub40")
    _, _, _, _, out1, g1 = _run(case)
    _, _, _, _, out2, g2 = _run(case)
    assert torch.equal(out1, out2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_two_pending_passes_through_graph_encoder_forward():
    """f(q) and f(k) forwarded by GraphEncoder.forward before one backward() of a loss that mixes them (an E2E step)"""
    enc = gat_encoder(hidden=32, heads=4, layers=2, T=2, Lr=2, pos=8, deg_emb=8, max_degree=16).cuda()
    views = [symmetric_batch([9, 4, 6], pos_dim=8, seed=20), symmetric_batch([5, 11, 3], pos_dim=8, seed=21)]
    r = torch.randn(3, 32, generator=torch.Generator().manual_seed(40))

    def loss_of(fq, fk):
        return (fq * fk).sum() + (fq * r.to(fq)).sum() - 2 * (fk * r.to(fk)).sum()

    fq, fk = enc(DeviceBatch(views[0])), enc(DeviceBatch(views[1]))
    assert fq.requires_grad and fk.requires_grad
    loss_of(fq, fk).backward()
    torch.cuda.synchronize()
    P = params_of(enc)
    loss_of(forward_of(enc, P, views[0]), forward_of(enc, P, views[1])).backward()
    worst, name = worst_rel_shared({k: v.grad for k, v in enc.named_parameters()}, {k: v.grad for k, v in P.items()})
    print(f"two pending passes on the device: worst gradient entry / scale {worst:.2e} ({name})")
    assert worst < GRAD_TOL, (worst, name)
