"""The GAT kernels (csrc/gat.hip) on the CPU emulator build at their shape edges (tests/gat_check.py: EDGE_CASES) against
the float64 restatement -- forward output and every parameter gradient --, the gradient metric where the true gradient
is zero, and the autograd glue (gcc_amd/autograd.py: _GatFn, gat_apply) that train.py --model gat, generate.py and
--finetune run: several passes pending at once, in-place updates, no_grad, frozen parameters, accumulation."""
import pytest
import torch

from gcc_amd.autograd import gat_apply
from gcc_amd.encoder import GatEngine
from tests.gat_check import (CASE_IDS, EDGE_CASES, case_inputs, dress_batch, gat_encoder, kernel_grads, reference_of,
                             symmetric_batch, worst_rel, worst_rel_shared)
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_encoder import CpuBatch

TOL = 2e-4          # tests/test_gat_emu.py's, for the output and for the gradients


def _engine():
    return GatEngine(lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr())


def _cpu_batch(batch, case):
    n = int(batch["node_off"][-1])
    return dress_batch(CpuBatch(batch, node_cap=max(n + case["cap_extra"], 1)), case)


@pytest.mark.parametrize("case", EDGE_CASES, ids=CASE_IDS)
def test_case_against_float64(case):
    enc, batch, dout, kw = case_inputs(case)
    g = _cpu_batch(batch, case)
    out, grads, _ = kernel_grads(enc, _engine(), g, dout)
    ref_out, ref_grads = reference_of(enc, batch, dout, kw)
    assert torch.isfinite(out).all()
    for k in ref_grads:
        assert torch.isfinite(grads[k]).all(), k
    out_err = float((out.double() - ref_out).abs().max())
    worst, name = worst_rel_shared(grads, ref_grads)
    print(f"{case['name']}: out err {out_err:.2e}; worst gradient entry / scale {worst:.2e} ({name})")
    torch.testing.assert_close(out.double(), ref_out, rtol=TOL, atol=TOL)
    bound = TOL
    if worst >= TOL:        # what float32 itself loses on these inputs (the rule of tests/test_gat_gpu.py), never on faith
        _, g32 = reference_of(enc, batch, dout, kw, dtype=torch.float32)
        worst32, name32 = worst_rel_shared(g32, ref_grads)
        print(f"{case['name']}: torch fp32 on the same inputs {worst32:.2e} ({name32})")
        bound = max(TOL, 2 * worst32)
    assert worst < bound, (worst, name, bound)


def test_shared_scale_only_moves_attn_r():
    """attn_r's true gradient cancels to zero in deep layers: its own max-abs is no scale.  The rule changes nothing else."""
    ref = {"gnn.layers.0.gnn.attn_l": torch.full((1, 2, 4), 1e-3, dtype=torch.float64),
           "gnn.layers.0.gnn.attn_r": torch.full((1, 2, 4), 1e-17, dtype=torch.float64),
           "gnn.layers.0.gnn.fc.weight": torch.full((8, 5), 2.0, dtype=torch.float64)}
    got = {k: v.clone() for k, v in ref.items()}
    got["gnn.layers.0.gnn.attn_r"] += 3e-8                        # float32 rounding of a sum whose terms are 1e-3
    assert worst_rel(got, ref)[0] > 1e8
    w, name = worst_rel_shared(got, ref)
    assert name == "gnn.layers.0.gnn.attn_r" and abs(w - 3e-5) < 1e-9
    got["gnn.layers.0.gnn.attn_r"] += 1e-6                        # a real error of 1e-3 of the shared scale is still seen
    assert worst_rel_shared(got, ref)[0] > 1e-3
    got = {k: v.clone() for k, v in ref.items()}
    got["gnn.layers.0.gnn.attn_l"] += 1e-6                        # attn_l and every other tensor: worst_rel's own scale
    got["gnn.layers.0.gnn.fc.weight"] += 1e-3
    assert worst_rel_shared(got, ref) == worst_rel(got, ref)
    ref["gnn.layers.0.gnn.attn_r"] = torch.full((1, 2, 4), 5.0, dtype=torch.float64)   # a live attn_r keeps its own scale
    got["gnn.layers.0.gnn.attn_r"] = ref["gnn.layers.0.gnn.attn_r"] + 1e-2
    assert worst_rel_shared(got, ref) == worst_rel(got, ref)


def test_null_col_idx_is_refused_by_name():
    """The C side keeps refusing a null col_idx (it cannot know the entry count without a sync), and says which member"""
    import ctypes

    enc = gat_encoder(hidden=32, heads=4, layers=2, T=2, Lr=1, pos=8, deg_emb=8, max_degree=16)
    g = CpuBatch(symmetric_batch([5, 3], pos_dim=8, seed=2))
    eng = _engine()
    out, saved, p, w = eng.forward(enc, g)
    p.col_idx = None
    rc = eng.lib.gcc_gat_forward(ctypes.byref(p), ctypes.byref(w), None)
    assert rc == -1 and "col_idx" in eng.lib.gcc_last_error().decode()


# ---- the autograd path: gat_apply on an encoder whose engine is the emulator's
def _api_encoder(**kw):
    enc = gat_encoder(**{**dict(hidden=32, heads=4, layers=2, T=2, Lr=2, pos=8, deg_emb=8, max_degree=16), **kw})
    enc._engine = _engine()
    return enc


def _views(k):
    sizes = [[9, 4, 6], [5, 11, 3], [7, 7, 2]]
    return [symmetric_batch(sizes[i], pos_dim=8, seed=20 + i) for i in range(k)]


def _mixed_loss(feats):
    """a loss that couples the passes (no one of them can be differentiated without the others' values) and weighs every
    output entry differently (the outputs are unit vectors: a plain sum of squares would be a constant)"""
    loss = 0.0
    for i, f in enumerate(feats):
        r = torch.randn(f.shape, generator=torch.Generator().manual_seed(40 + i)).to(f.dtype)
        loss = loss + (f * r).sum()
        if len(feats) > 1:
            loss = loss + (i + 1) * (f * feats[(i + 1) % len(feats)]).sum()
    return loss


def _float64_grads(enc, views):
    from tests.gat_reference import forward_of, params_of

    P = params_of(enc)
    _mixed_loss([forward_of(enc, P, v) for v in views]).backward()
    return {k: v.grad for k, v in P.items()}


@pytest.mark.parametrize("passes", [2, 3])
def test_pending_passes_share_one_backward(passes):
    """f(q), f(k) (and a third) are all forwarded before one backward(): the engine keeps no state between passes"""
    enc = _api_encoder()
    views = _views(passes)
    feats = [gat_apply(enc, CpuBatch(v)) for v in views]
    assert all(f.requires_grad for f in feats)
    _mixed_loss(feats).backward()
    worst, name = worst_rel_shared({k: v.grad for k, v in enc.named_parameters()}, _float64_grads(enc, views))
    print(f"{passes} pending passes: worst gradient entry / scale {worst:.2e} ({name})")
    assert worst < TOL, (worst, name)


def test_in_place_update_between_forward_and_backward_raises():
    enc = _api_encoder()
    f = gat_apply(enc, CpuBatch(_views(1)[0]))
    with torch.no_grad():
        enc.lin_readout[2].weight.mul_(0.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        f.sum().backward()


def test_no_grad_builds_no_node():
    enc = _api_encoder()
    g = CpuBatch(_views(1)[0])
    with torch.no_grad():
        f = gat_apply(enc, g)
    assert not f.requires_grad and f.grad_fn is None
    assert torch.equal(f, gat_apply(enc, g).detach())


def test_frozen_parameter_keeps_no_grad():
    enc = _api_encoder()
    frozen = ["gnn.layers.0.gnn.fc.weight", "set2set.lstm.bias_hh_l1", "degree_embedding.weight"]
    named = dict(enc.named_parameters())
    for k in frozen:
        named[k].requires_grad_(False)
    views = _views(1)
    _mixed_loss([gat_apply(enc, CpuBatch(views[0]))]).backward()
    ref = _float64_grads(enc, views)
    for k in frozen:
        assert named[k].grad is None, k
        del ref[k]
    worst, name = worst_rel_shared({k: named[k].grad for k in ref}, ref)
    assert worst < TOL, (worst, name)


def test_second_backward_accumulates_exactly():
    enc = _api_encoder()
    f = gat_apply(enc, CpuBatch(_views(1)[0]))
    loss = _mixed_loss([f])
    loss.backward(retain_graph=True)
    first = {k: v.grad.clone() for k, v in enc.named_parameters()}
    loss.backward()
    for k, v in enc.named_parameters():
        assert torch.equal(v.grad, 2 * first[k]), k
