"""The any-width encoder (csrc/ginx.hip) and the wide head at the edges the sampled batches of the other tests never reach, each
against oracle/encoder.py run in float64.  Emulator tier; the device tier is tests/test_wide_step_gpu.py.

- widths that are not multiples of four through the fused step (MoCoTrainStep._body on the any-width engines): parameters at offsets of the flat
  buffer that are not 16-byte aligned, so the GEMM's, BatchNorm's, pooling's and spmm's scalar paths run on them;
- a width above 256 through the API path: the 256-column loops of spmm, pooling and the column sums take a second trip;
- hand-built batches of 1023, 1024, 1025 and 2049 live rows (the weight gradients' 1,024-row slabs and the end of the last one)
  inside a larger node capacity whose rows past the live count hold a larger earlier batch's activations and gradients, with
  NaN in the dead input rows, empty and one-node subgraphs, isolated nodes and a node whose degree exceeds max_degree;
- a degree-embedding table too large for LDS (the global-atomic branch of ginx_feat_bwd_kernel);
- the wide head at D = 65, 130 on both sides of its long-reduction split (K = 4096)."""
import numpy as np
import pytest
import torch

from gcc_amd.contrast import MemoryMoCo, NCESoftmaxLoss
from gcc_amd.encoder import GraphEncoder
from gcc_amd.train_step import MoCoTrainStep
from oracle import encoder as E
from tests.hipemu.emu_encoder import CpuBatch
from tests.test_nce_emu import emu_nce
from tests.test_wide_encoder_emu import emu_wide_engine, emu_wide_nce, fixed_views
from tests.wide_step_check import check_wide_moco_step, grad_bar, oracle_like

B = 24


def encoder(hidden, out, layers, max_degree=512, degree_embedding_size=16):
    return GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=max_degree,
                        freq_embedding_size=16, degree_embedding_size=degree_embedding_size, output_dim=out,
                        node_hidden_dim=hidden, edge_hidden_dim=hidden, num_layers=layers, num_step_set2set=6,
                        num_layer_set2set=3, norm=True, gnn_model="gin", degree_input=True)


def hand_batch(n_live, node_cap, seed, hub_degree=0):
    """B subgraphs over ``n_live`` nodes inside ``node_cap`` rows: the first and the last subgraph empty, two of one node, one
    star whose centre has ``hub_degree`` neighbours (when > 0), the rest random symmetric graphs of mean degree ~3 whose last
    node is isolated.  Rows past the live count: NaN positional embedding, zero CSR."""
    rng = np.random.default_rng(seed)
    fixed = [1, 1] + ([hub_degree + 1] if hub_degree else [])
    nrand = B - 2 - len(fixed)
    left = n_live - sum(fixed)
    assert left >= 3 * nrand
    cuts = np.sort(rng.choice(np.arange(1, left // 3), nrand - 1, replace=False)) * 3
    mid = fixed + [int(s) for s in np.diff(np.concatenate([[0], cuts, [left]]))]
    rng.shuffle(mid)
    sizes = [0] + mid + [0]
    node_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    adj = [set() for _ in range(n_live)]
    for b, s in enumerate(sizes):
        o = int(node_off[b])
        if s == hub_degree + 1 and hub_degree:
            for v in range(1, s):
                adj[o].add(o + v)
                adj[o + v].add(o)
        elif s > 2:
            for _ in range(int(1.5 * (s - 1))):
                u, v = rng.integers(0, s - 1, 2)          # (node s - 1 stays isolated)
                if u != v:
                    adj[o + u].add(o + v)
                    adj[o + v].add(o + u)
    row_ptr = np.concatenate([[0], np.cumsum([len(a) for a in adj])]).astype(np.int64)
    col_idx = np.concatenate([sorted(a) for a in adj if a]).astype(np.int64)
    pos = torch.nn.functional.normalize(torch.randn(n_live, 32, generator=torch.Generator().manual_seed(seed)), dim=1)
    g = CpuBatch(dict(node_off=torch.from_numpy(node_off), row_ptr=torch.from_numpy(row_ptr), col_idx=torch.from_numpy(col_idx),
                      pos_undirected=pos), node_cap=node_cap)
    g.pos_undirected[n_live:] = float("nan")
    assert g.batch_size == B and int(g.node_off[B]) == n_live and g.graph_id.numel() == node_cap > n_live
    return g


class _ScriptedSampler:
    """step i's views: ``steps[i]``"""
    batch_size = B

    def __init__(self, steps):
        self.steps = steps

    def sample(self, first_id, prof=None):
        return self.steps[first_id // B]


def _fused_step(hidden, out, layers, steps, K=96, **kw):
    torch.manual_seed(hidden * 1000 + out)
    model, ema = encoder(hidden, out, layers, **kw), encoder(hidden, out, layers, **kw)
    ema.load_state_dict(model.state_dict())
    model._wide_engine = ema._wide_engine = emu_wide_engine()
    contrast = MemoryMoCo(out, None, K, 0.07, use_softmax=True)
    contrast._engine = emu_wide_nce()
    tr = MoCoTrainStep(model, ema, contrast, _ScriptedSampler(steps), posemb=lambda gr: gr, prefetch=False, flat_engine=emu_nce())
    assert tr.wide and not tr.use_graph
    return tr, model, ema, contrast


def _masks(layers, out, seed):
    return (torch.rand(layers, B, out, generator=torch.Generator().manual_seed(seed)) >= 0.5).float().contiguous()


@pytest.mark.parametrize("hidden,out", [(66, 66), (130, 65)])
def test_fused_step_at_widths_off_the_16_byte_grid(hidden, out):
    layers = 3
    tr, model, ema, contrast = _fused_step(hidden, out, layers, [fixed_views()])
    # the flat parameter buffer puts GEMM operands (Linear weights) and BatchNorm parameters at offsets that are not 16-byte aligned
    gin = model.gnn.ginlayers
    operands = [ly.apply_func.mlp.linears[j].weight for ly in gin for j in (0, 1)] + [lin.weight for lin in model.gnn.linears_prediction]
    assert any(w.data_ptr() % 16 for w in operands), "no GEMM operand is misaligned: the case lost its point"
    bns = [ly.apply_func.bn.weight for ly in gin] + [bn.weight for bn in model.gnn.batch_norms]
    assert any(w.data_ptr() % 16 for w in bns)
    rep = check_wide_moco_step(tr, model, ema, contrast, 0.004, _masks(layers, out, hidden), step_id=0)
    print(f"{hidden}/{out}: worst gradient entry vs float64 {rep['grad_err_vs_f64_step']:.2e} (torch fp32 "
          f"{rep['grad_err_vs_f64_torch32']:.2e}) of the tensor's largest entry")


def test_api_path_above_256_columns(monkeypatch):
    """hidden = out = 320: every 256-column loop (spmm, pooling, column sums, normalisation) takes a second, partial trip"""
    from tests.test_wide_encoder_emu import check_against_oracle

    hidden = out = 320
    layers = 2
    torch.manual_seed(320)
    model = encoder(hidden, out, layers)
    oracle = E.OracleGraphEncoder(node_hidden_dim=hidden, output_dim=out, num_layers=layers)
    oracle.load_state_dict(model.state_dict())
    model._wide_engine = emu_wide_engine()
    model.train()
    oracle.train()
    q, _ = fixed_views()
    check_against_oracle(model, oracle, q, _masks(layers, out, 3), out, hidden, monkeypatch)


@pytest.mark.parametrize("n_live", [1023, 1024, 1025, 2049])
def test_fused_step_on_hand_built_batches_over_stale_rows(n_live):
    """node_cap 2,112 for every case; the first step runs a 2,100-row batch through the same workspaces (forward, backward), so the
    rows between the live count and the capacity hold its activations and gradients; the checked step is the second"""
    hidden, out, layers, cap = 66, 66, 2, 2112
    big = (hand_batch(2100, cap, 1, hub_degree=600), hand_batch(2100, cap, 2))
    test = (hand_batch(n_live, cap, 10 + n_live, hub_degree=530), hand_batch(n_live, cap, 20 + n_live))
    tr, model, ema, contrast = _fused_step(hidden, out, layers, [big, test])
    tr.mask_fn = lambda: _masks(layers, out, 5)
    tr.step(0, 0.005)
    rep = check_wide_moco_step(tr, model, ema, contrast, 0.004, _masks(layers, out, 6), step_id=1)
    assert rep["nodes_q"] == rep["nodes_k"] == n_live
    print(f"{n_live} live rows: worst gradient entry vs float64 {rep['grad_err_vs_f64_step']:.2e} "
          f"(torch fp32 {rep['grad_err_vs_f64_torch32']:.2e})")


def test_degree_embedding_table_larger_than_lds(monkeypatch):
    """max_degree 1023 x 16 columns = 16,384 floats > the 10,240 of ginx_feat_bwd_kernel's LDS copy: the scatter-add goes straight
    to global memory.  A 1,100-neighbour hub is clamped to row 1,023.  (Such a hub is an outlier every BatchNorm of the layer sees:
    on some seeds of this batch one pre-activation sits within fp32 rounding of a ReLU kink, and then the kernels and torch's fp32
    run are off from float64 by the same 1e-3 of a tensor's scale.  This seed keeps torch's fp32 run inside the bar too.)"""
    hidden, out, layers = 72, 72, 2
    torch.manual_seed(1023)
    model = encoder(hidden, out, layers, max_degree=1023, degree_embedding_size=16)
    assert (model.max_degree + 1) * model.degree_embedding_size > 10240
    model._wide_engine = emu_wide_engine()
    model.train()
    g = hand_batch(2049, 2112, 3, hub_degree=1100)
    keep = _masks(layers, out, 8)
    monkeypatch.setattr(torch, "rand", lambda *a, **kw: keep.clone())
    o64 = oracle_like(model, torch.float64)
    o64.train()
    feat = model(g)
    n = int(g.node_off[B])
    args = (g.node_off.long(), g.row_ptr[: n + 1].long(), g.col_idx.long())
    ref = o64(*args, g.pos_undirected[:n].double(), dropout_masks=keep.double())
    torch.testing.assert_close(feat.double(), ref.detach(), rtol=2e-4, atol=2e-5)
    d = torch.randn(B, out, generator=torch.Generator().manual_seed(9))
    feat.backward(d)
    ref.backward(d.double())
    demb = o64.degree_embedding.weight.grad
    rows = (demb.abs().sum(1) > 0).nonzero().flatten()
    assert int(rows.max()) == 1023 and len(rows) >= 4           # the clamped hub and several small degrees
    ref64 = dict(o64.named_parameters())
    for name, p in model.named_parameters():
        if ref64[name].grad is None:
            continue
        g64 = ref64[name].grad
        scale, atol = grad_bar(name, g64)
        err = float((p.grad.double() - g64).abs().max())
        assert err <= atol, f"d {name}: {err:.3e} from float64 (bar {atol:.3e})"


@pytest.mark.parametrize("D", [65, 130])
@pytest.mark.parametrize("K", [4096, 4097, 8192])
def test_wide_head_off_grid_widths_and_long_queues(D, K):
    """MemoryMoCo(D, K) on the dense head: logits, loss, prob, d loss / d q against float64 (K >= 4096: the reduction over the
    queue is split over workgroups with fp64 atomics), the queue after the enqueue, over two steps"""
    torch.manual_seed(D * K)
    Bq = 40
    contrast = MemoryMoCo(D, None, K, 0.07, use_softmax=True)
    contrast._engine = emu_wide_nce()
    mem = contrast.memory.clone().double()
    index = K - 17                                                # the second step's keys wrap around the ring
    contrast.index = index
    for step in range(2):
        q = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1).requires_grad_()
        k = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1)
        q64 = q.detach().double().requires_grad_()
        out = contrast(q, k)
        loss = NCESoftmaxLoss()(out)
        loss.backward()
        ref_out, new_index = E.moco_forward(mem, index, q64, k.double(), 0.07)
        ref_loss = E.nce_softmax_loss(ref_out)
        ref_loss.backward()
        torch.testing.assert_close(out.dense().double(), ref_out.detach(), rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(loss.detach().double(), ref_loss.detach(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(out.prob.double(), ref_out[:, 0].mean().detach(), rtol=1e-5, atol=1e-5)
        scale = float(q64.grad.abs().max())
        torch.testing.assert_close(q.grad.double(), q64.grad, rtol=1e-3, atol=1e-3 * scale)
        torch.testing.assert_close(contrast.memory.double(), mem, rtol=0, atol=0)
        index = new_index
        assert contrast.index == index
