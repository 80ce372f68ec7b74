"""Shared by the edge tests of the any-width encoder and the dense head (csrc/ginx.hip): ONE set of case builders and check
bodies, run by the emulator tier (tests/test_wide_edges_emu.py, tests/test_wide_bf16_emu.py, tests/test_wide_encoder_emu.py) and by
the device tier (tests/test_wide_edges_gpu.py, tests/test_wide_bf16_edges_gpu.py).  TEST INFRASTRUCTURE ONLY.

A :class:`Tier` selects the engine factories (the emulator library on CPU tensors, or the gfx950 library on ``cuda`` tensors),
the batch class and a ``sync`` callable.  Inputs are ALWAYS generated on the CPU from fixed seeds and then moved; models are
initialised on the CPU under ``torch.manual_seed`` and then moved: both tiers run the same numbers.

Bars: none are chosen here.  f32: features rtol 2e-4 / atol 2e-5, pooled outputs atol 2e-4, gradients ``grad_bar`` (1e-3 of the
tensor's largest entry against float64), the head's own bars.  bf16: :class:`tests.wide_bf16_step_check.Bars` -- the f32-mode value
or twice the rounded oracle's fp32-vs-float64 gap, whichever is larger; the gap is measured on the reference, never on the code
under test.  Every body also asserts the REFERENCE condition: torch's fp32 run of the oracle stays inside the gradient bar
against its float64 run (``assert_reference_inside_bar``), so an input with a pre-activation on a ReLU kink fails as a bad
input, not as a wrong kernel."""
import copy

import numpy as np
import torch

from gcc_amd.contrast import MemoryMoCo, NceEngine, NCESoftmaxLoss, NCESoftmaxLossNS, WideNceEngine, e2e_logits
from gcc_amd.encoder import GraphEncoder
from gcc_amd.encoder_wide import WideGinEngine
from gcc_amd.train_step import MoCoTrainStep
from oracle import encoder as E
from tests import bf16_reference as R
from tests.hipemu.emu_encoder import CpuBatch
from tests.wide_bf16_step_check import Bars, check_wide_bf16_moco_step
from tests.wide_step_check import check_wide_moco_step, grad_bar, oracle_like

B = 24


class Tier:
    """``emu``: the wave64 emulator build on CPU tensors (CpuBatch); ``gpu``: the gfx950 library on ``cuda`` tensors
    (gcc_amd.sampler.BatchedCSR with every member the engines and the step read, capacity-sized)."""

    def __init__(self, name):
        assert name in ("emu", "gpu"), name
        self.name = name
        self.device = "cpu" if name == "emu" else "cuda"

    def _kw(self):
        if self.name == "gpu":
            return {}
        from tests.hipemu.emu_driver import emu_lib

        return dict(lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr())

    def wide_engine(self):
        return WideGinEngine(**self._kw())

    def wide_nce(self, dtype="f32"):
        return WideNceEngine(dtype=dtype, **self._kw())

    def flat_engine(self):
        return NceEngine(**self._kw())

    def gin_engine(self):
        """the fused 64-channel GIN pass (csrc/encoder.hip, encoder_bwd.hip)"""
        from gcc_amd.encoder import GinEngine

        return GinEngine(**self._kw())

    def head_engine(self):
        """the fine-tuning head and clip-by-value Adam (csrc/cls_head.hip, csrc/step_tail.hip)"""
        from gcc_amd.finetune import ClsHeadEngine

        return ClsHeadEngine(**self._kw())

    def sync(self):
        if self.name == "gpu":
            torch.cuda.synchronize()

    def to(self, t):
        """a CPU tensor or module on the tier's device"""
        return t.to(self.device)

    def batch(self, g):
        """a CpuBatch as the tier's batch: itself, or a BatchedCSR holding the SAME arrays on the device -- real graph_id
        (ginx_pool_bwd_kernel indexes with it), row_ptr of capacity + 1 entries, whatever the dead rows of pos_undirected hold"""
        if self.name == "emu":
            return g
        from gcc_amd.sampler import BatchedCSR

        d = self.device
        out = BatchedCSR(g.batch_size, g.node_off.to(d), g.edge_off.to(d), g.parent_nid.to(d), g.graph_id.to(d),
                         g.row_ptr.to(d), g.col_idx.to(d))
        out.pos_undirected = g.pos_undirected.to(d)
        assert out.parent_nid.numel() == out.graph_id.numel() == out.pos_undirected.shape[0] == out.row_ptr.numel() - 1
        return out


EMU, GPU = Tier("emu"), Tier("gpu")


def live_rows(g):
    return int(g.node_off[g.batch_size])


# ---------------------------------------------------------------------------------------------------------------------
# builders
def encoder(hidden, out, layers, max_degree=512, degree_embedding_size=16, **kw):
    return GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=max_degree,
                        freq_embedding_size=16, degree_embedding_size=degree_embedding_size, output_dim=out,
                        node_hidden_dim=hidden, edge_hidden_dim=hidden, num_layers=layers, num_step_set2set=6,
                        num_layer_set2set=3, norm=True, gnn_model="gin", degree_input=True, **kw)


def fixed_views(tier=EMU):
    """The sampled batch of the headline tests with a REPRODUCIBLE positional embedding: OracleSampler's comes from SciPy ARPACK, whose
    output differs from call to call (the degenerate eigenspaces of small ego-nets), and with ~2 M pre-activations per pass an input
    now and then puts one of them within fp32 rounding of a ReLU kink -- then ANY two fp32 implementations may disagree on that
    element's mask and its whole upstream gradient (seen: 1e-2 of a gradient's scale, one element with |y| < 1e-6 in float64).  Unit rows
    from a seeded generator keep the test's inputs, and so its verdict, the same on every run."""
    from tests.test_headline_step_emu import OracleSampler

    q, k = OracleSampler().views
    for v, seed in ((q, 11), (k, 12)):
        x = torch.randn(v.pos_undirected.shape, generator=torch.Generator().manual_seed(seed))
        v.pos_undirected = torch.nn.functional.normalize(x, dim=1)
    return tier.batch(q), tier.batch(k)


def hand_batch(n_live, node_cap, seed, hub_degree=0, tier=EMU):
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
    g = tier.batch(g)
    assert bool(torch.isnan(g.pos_undirected[n_live:]).all()) and int(g.graph_id[:n_live].max()) == B - 2
    return g


class ScriptedSampler:
    """step i's views: ``steps[i]``"""
    batch_size = B

    def __init__(self, steps):
        self.steps = steps

    def sample(self, first_id, prof=None):
        return self.steps[first_id // B]


def masks(layers, out, seed, tier=EMU):
    return tier.to((torch.rand(layers, B, out, generator=torch.Generator().manual_seed(seed)) >= 0.5).float().contiguous())


def fused_step(hidden, out, layers, steps, K=96, tier=EMU, seed=None, nce_dtype="f32", **kw):
    """MoCoTrainStep on the any-width engines of ``tier`` over scripted views -> (trainer, model, ema, contrast)"""
    torch.manual_seed(hidden * 1000 + out if seed is None else seed)
    model, ema = encoder(hidden, out, layers, **kw), encoder(hidden, out, layers, **kw)
    ema.load_state_dict(model.state_dict())
    contrast = MemoryMoCo(out, None, K, 0.07, use_softmax=True, nce_dtype=nce_dtype)
    model, ema, contrast = tier.to(model), tier.to(ema), tier.to(contrast)
    model._wide_engine = ema._wide_engine = tier.wide_engine()
    contrast._engine = tier.wide_nce(nce_dtype)
    tr = MoCoTrainStep(model, ema, contrast, ScriptedSampler(steps), posemb=lambda gr: gr, prefetch=False,
                       flat_engine=tier.flat_engine())
    assert tr.wide and not tr.use_graph and tr.nce.dtype == nce_dtype
    return tr, model, ema, contrast


def assert_reference_inside_bar(rep, what):
    """the reference condition of a fused-step case: torch's fp32 run of the oracle is inside the gradient bar (1e-3 of each
    tensor's largest entry) against its float64 run"""
    e32 = rep["grad_err_vs_f64_torch32"]
    assert e32 <= 1e-3, f"{what}: BAD INPUT, not a kernel error -- torch's fp32 run of the oracle is {e32:.2e} of a tensor's " \
                        f"largest entry from float64 (bar 1e-3): a pre-activation sits on a ReLU kink"


def assert_resolution(bars, what, limit=1e-3, show=True):
    """For every kind of quantity whose rule gap is below ``limit``: the bar each comparison was held to is the f32-mode value
    or twice that measured gap, nothing wider, and the error is inside it.  Prints error | gap per kind; -> {kind: (err, gap)}"""
    fig = {}
    for kind in dict.fromkeys(r["kind"] for r in bars.rows):
        err, gap = bars.worst(kind)
        fig[kind] = (err, gap)
        if show:
            print(f"{what}: {kind} err {err:.2e} | rule gap {gap:.2e}" + ("" if gap < limit else "   (gap above %.0e)" % limit))
        if gap < limit:
            for r in (r for r in bars.rows if r["kind"] == kind):
                assert bars.bar(r) <= max(r["atol"], 2.0 * gap) and bars.bar(r) < max(r["atol"], 2.0 * limit), r
                assert r["excess"] <= bars.bar(r), r
    return fig


# ---------------------------------------------------------------------------------------------------------------------
# f32 bodies: against oracle/encoder.py in float64
def check_fused_step_off_grid(tier, hidden, out):
    """the fused step at a width that is no multiple of four: misaligned operands in the flat parameter buffer"""
    layers = 3
    tr, model, ema, contrast = fused_step(hidden, out, layers, [fixed_views(tier)], tier=tier)
    # the flat parameter buffer puts GEMM operands (Linear weights) and BatchNorm parameters at offsets that are not 16-byte aligned
    gin = model.gnn.ginlayers
    operands = [ly.apply_func.mlp.linears[j].weight for ly in gin for j in (0, 1)] + [lin.weight for lin in model.gnn.linears_prediction]
    assert any(w.data_ptr() % 16 for w in operands), "no GEMM operand is misaligned: the case lost its point"
    bns = [ly.apply_func.bn.weight for ly in gin] + [bn.weight for bn in model.gnn.batch_norms]
    assert any(w.data_ptr() % 16 for w in bns)
    rep = check_wide_moco_step(tr, model, ema, contrast, 0.004, masks(layers, out, hidden, tier), sync=tier.sync, step_id=0)
    print(f"{hidden}/{out}: worst gradient entry vs float64 {rep['grad_err_vs_f64_step']:.2e} (torch fp32 "
          f"{rep['grad_err_vs_f64_torch32']:.2e}) of the tensor's largest entry")
    assert_reference_inside_bar(rep, f"{hidden}/{out}")
    return rep


def check_stale_rows_step(tier, n_live):
    """node_cap 2,112 for every case; the first step runs a 2,100-row batch through the same workspaces (forward, backward), so the
    rows between the live count and the capacity hold its activations and gradients; the checked step is the second"""
    hidden, out, layers, cap = 66, 66, 2, 2112
    big = (hand_batch(2100, cap, 1, hub_degree=600, tier=tier), hand_batch(2100, cap, 2, tier=tier))
    test = (hand_batch(n_live, cap, 10 + n_live, hub_degree=530, tier=tier), hand_batch(n_live, cap, 20 + n_live, tier=tier))
    tr, model, ema, contrast = fused_step(hidden, out, layers, [big, test], tier=tier)
    tr.mask_fn = lambda: masks(layers, out, 5, tier)
    tr.step(0, 0.005)
    rep = check_wide_moco_step(tr, model, ema, contrast, 0.004, masks(layers, out, 6, tier), sync=tier.sync, step_id=1)
    assert rep["nodes_q"] == rep["nodes_k"] == n_live
    print(f"{n_live} live rows: worst gradient entry vs float64 {rep['grad_err_vs_f64_step']:.2e} "
          f"(torch fp32 {rep['grad_err_vs_f64_torch32']:.2e})")
    assert_reference_inside_bar(rep, f"{n_live} live rows")
    return rep


def _oracle_args(q, nb):
    n = live_rows(q)
    return (q.node_off.long().cpu(), q.row_ptr[: n + 1].long().cpu(), q.col_idx.long().cpu(), q.pos_undirected[:n].cpu())


def check_against_oracle(model, oracle, q, keep, out, hidden, monkeypatch, rtol=2e-4, nb=B, tier=EMU, reference_bar=True):
    """ONE training-mode pass of ``model`` (API path) on ``q``: features and pooled outputs against the fp32 oracle, every
    parameter gradient against the float64 oracle -> (the oracle's arguments, worst gradient error, worst torch-fp32 error:
    both of the tensor's largest entry against float64).  ``keep`` (CPU) is the dropout masks of both sides.
    ``reference_bar``: assert that torch's fp32 run is inside the gradient bar too."""
    keep_dev = tier.to(keep)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: keep_dev.clone())       # the API path draws its dropout masks here
    feat, pooled = model(q, return_all_outputs=True)
    assert tuple(feat.shape) == (nb, out) and all(tuple(t.shape) == (nb, hidden) for t in pooled)
    args = _oracle_args(q, nb)
    ref, ref_pooled = oracle(*args, dropout_masks=keep, return_all_outputs=True)
    torch.testing.assert_close(feat.detach().cpu(), ref.detach(), rtol=rtol, atol=2e-5)
    for a, b in zip(pooled, ref_pooled):
        torch.testing.assert_close(a.detach().cpu(), b.detach(), rtol=rtol, atol=2e-4)
    d = torch.randn(nb, out)
    feat.backward(tier.to(d))
    tier.sync()
    ref.backward(d)
    refg = dict(oracle.named_parameters())
    # the binding reference for the gradients is the same model in float64: a weight gradient sums thousands of terms that largely cancel,
    # so two fp32 implementations (the kernels, torch's) differ from each other by what each is off from float64.  The bar: 1e-3 of the
    # tensor's largest entry against the float64 run (north_star), no allowance for fp32
    o64 = copy.deepcopy(oracle).double()
    o64.zero_grad()
    r64 = o64(args[0], args[1], args[2], args[3].double(), dropout_masks=keep.double(), return_all_outputs=True)[0]
    r64.backward(d.double())
    ref64 = dict(o64.named_parameters())
    worst, worst32, name32 = 0.0, 0.0, None
    for name, p in model.named_parameters():
        if refg[name].grad is None:
            assert p.grad is None or float(p.grad.abs().sum()) == 0.0, name
            continue
        assert p.grad.shape == p.shape
        g64 = ref64[name].grad.float()
        scale = max(float(g64.abs().max()), 1e-3)
        worst = max(worst, float((p.grad.cpu() - g64).abs().max()) / scale)
        # (the reference condition is held to grad_bar: where the exact gradient is zero -- the bias of a Linear in front of a
        #  BatchNorm -- torch's fp32 value is rounding noise, 1e-6 absolute, and no sign of a ReLU kink)
        e32 = float((refg[name].grad - g64).abs().max()) / grad_bar(name, ref64[name].grad)[0]
        if e32 > worst32:
            worst32, name32 = e32, name
        torch.testing.assert_close(p.grad.cpu(), g64, rtol=0, atol=1e-3 * scale, msg=lambda m, name=name: f"{name}: {m}")
    print(f"{hidden}/{out}: worst gradient entry vs float64 {worst:.2e} (torch fp32 {worst32:.2e}, {name32}) of the tensor's largest entry")
    if reference_bar:
        assert worst32 <= 1e-3, f"BAD INPUT, not a kernel error: torch's fp32 d {name32} is {worst32:.2e} from float64 (bar 1e-3)"
    return args, worst, worst32


def check_api_above_256(tier, monkeypatch):
    """hidden = out = 320: every 256-column loop (spmm, pooling, column sums, normalisation) takes a second, partial trip"""
    hidden = out = 320
    layers = 2
    torch.manual_seed(320)
    model = encoder(hidden, out, layers)
    oracle = E.OracleGraphEncoder(node_hidden_dim=hidden, output_dim=out, num_layers=layers)
    oracle.load_state_dict(model.state_dict())
    model = tier.to(model)
    model._wide_engine = tier.wide_engine()
    model.train()
    oracle.train()
    q, _ = fixed_views(tier)
    keep = (torch.rand(layers, B, out, generator=torch.Generator().manual_seed(3)) >= 0.5).float().contiguous()
    return check_against_oracle(model, oracle, q, keep, out, hidden, monkeypatch, tier=tier)


def check_api_path(tier, hidden, out, layers, monkeypatch, reference_bar=True):
    """API path in f32: training forward and backward, running statistics, save / load, eval mode, embed_views"""
    torch.manual_seed(hidden * 100 + out)
    model = encoder(hidden, out, layers)
    assert model.wide and not model.is_padded()
    oracle = E.OracleGraphEncoder(node_hidden_dim=hidden, output_dim=out, num_layers=layers)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in oracle.state_dict().items()}
    oracle.load_state_dict(model.state_dict())
    model = tier.to(model)
    model._wide_engine = tier.wide_engine()
    model.train()
    oracle.train()
    q, _ = fixed_views(tier)
    keep = (torch.rand(layers, B, out) >= 0.5).float()
    args, worst, worst32 = check_against_oracle(model, oracle, q, keep, out, hidden, monkeypatch, tier=tier, reference_bar=reference_bar)
    # running statistics moved exactly as torch's BatchNorm1d moves them (momentum 0.1, unbiased variance)
    for (k1, v1), (k2, v2) in zip(model.state_dict().items(), oracle.state_dict().items()):
        if "running_" in k1 or "num_batches" in k1:
            torch.testing.assert_close(v1.cpu(), v2, rtol=1e-4, atol=1e-5, msg=lambda m, k=k1: f"{k}: {m}")
    # the state survives a save / load round trip, and eval mode (running statistics, no dropout) agrees too
    m2 = encoder(hidden, out, layers)
    m2.load_state_dict({k: v.cpu().clone() for k, v in model.state_dict().items()})
    m2 = tier.to(m2)
    m2._wide_engine = tier.wide_engine()
    m2.eval()
    oracle.eval()
    with torch.no_grad():
        torch.testing.assert_close(m2(q).cpu(), oracle(*args), rtol=2e-4, atol=2e-5)
        torch.testing.assert_close(m2.embed_views(q, q).cpu(), oracle(*args), rtol=2e-4, atol=2e-5)
    return worst, worst32


def check_degree_table(tier, monkeypatch):
    """max_degree 1023 x 16 columns = 16,384 floats > the 10,240 of ginx_feat_bwd_kernel's LDS copy: the scatter-add goes straight
    to global memory.  A 1,100-neighbour hub is clamped to row 1,023.  (Such a hub is an outlier every BatchNorm of the layer sees:
    on some seeds of this batch one pre-activation sits within fp32 rounding of a ReLU kink, and then the kernels and torch's fp32
    run are off from float64 by the same 1e-3 of a tensor's scale.  This seed keeps torch's fp32 run inside the bar too -- which
    the body asserts.)  -> (worst gradient error, worst torch-fp32 error) of the tensor's largest entry against float64"""
    hidden, out, layers = 72, 72, 2
    torch.manual_seed(1023)
    model = encoder(hidden, out, layers, max_degree=1023, degree_embedding_size=16)
    assert (model.max_degree + 1) * model.degree_embedding_size > 10240
    o32, o64 = oracle_like(model, torch.float32), oracle_like(model, torch.float64)
    model = tier.to(model)
    model._wide_engine = tier.wide_engine()
    model.train()
    g = hand_batch(2049, 2112, 3, hub_degree=1100, tier=tier)
    keep = masks(layers, out, 8)
    keep_dev = tier.to(keep)
    monkeypatch.setattr(torch, "rand", lambda *a, **kw: keep_dev.clone())
    o32.train()
    o64.train()
    feat = model(g)
    args = _oracle_args(g, B)
    ref = o64(args[0], args[1], args[2], args[3].double(), dropout_masks=keep.double())
    ref32 = o32(*args, dropout_masks=keep)
    torch.testing.assert_close(feat.detach().cpu().double(), ref.detach(), rtol=2e-4, atol=2e-5)
    d = torch.randn(B, out, generator=torch.Generator().manual_seed(9))
    feat.backward(tier.to(d))
    tier.sync()
    ref.backward(d.double())
    ref32.backward(d)
    demb = o64.degree_embedding.weight.grad
    rows = (demb.abs().sum(1) > 0).nonzero().flatten()
    assert int(rows.max()) == 1023 and len(rows) >= 4           # the clamped hub and several small degrees
    ref64, r32 = dict(o64.named_parameters()), dict(o32.named_parameters())
    worst, worst32 = 0.0, 0.0
    for name, p in model.named_parameters():
        if ref64[name].grad is None:
            continue
        g64 = ref64[name].grad
        scale, atol = grad_bar(name, g64)
        err = float((p.grad.cpu().double() - g64).abs().max())
        e32 = float((r32[name].grad.double() - g64).abs().max())
        worst, worst32 = max(worst, err / scale), max(worst32, e32 / scale)
        assert e32 <= atol, f"BAD INPUT, not a kernel error: torch's fp32 d {name} is {e32:.3e} from float64 (bar {atol:.3e})"
        assert err <= atol, f"d {name}: {err:.3e} from float64 (bar {atol:.3e})"
    print(f"degree table 1023 x 16: worst gradient entry vs float64 {worst:.2e} (torch fp32 {worst32:.2e})")
    return worst, worst32


def _ring_start(K, Bq):
    return K - min(17, Bq)                       # the second step's keys wrap around the ring


def check_head(tier, D, K, Bq=40):
    """MemoryMoCo(D, K) on the dense head: logits, loss, prob, d loss / d q against float64 (K >= 4096: the reduction over the
    queue is split over workgroups with fp64 atomics), the queue after the enqueue exactly, over two steps with a wrapping ring
    pointer.  -> worst d q error of its largest entry"""
    torch.manual_seed(D * K)
    contrast = MemoryMoCo(D, None, K, 0.07, use_softmax=True)
    mem = contrast.memory.clone().double()
    contrast = tier.to(contrast)
    contrast._engine = tier.wide_nce()
    index = _ring_start(K, Bq)
    contrast.index = index
    worst = 0.0
    for step in range(2):
        q0 = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1)
        k = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1)
        q = tier.to(q0).clone().requires_grad_()
        q64 = q0.double().requires_grad_()
        out = contrast(q, tier.to(k))
        loss = NCESoftmaxLoss()(out)
        loss.backward()
        tier.sync()
        ref_out, new_index = E.moco_forward(mem, index, q64, k.double(), 0.07)
        ref_loss = E.nce_softmax_loss(ref_out)
        ref_loss.backward()
        torch.testing.assert_close(out.dense().cpu().double(), ref_out.detach(), rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(loss.detach().cpu().double(), ref_loss.detach(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(out.prob.cpu().double().reshape(()), ref_out[:, 0].mean().detach(), rtol=1e-5, atol=1e-5)
        scale = float(q64.grad.abs().max())
        worst = max(worst, float((q.grad.cpu().double() - q64.grad).abs().max()) / scale)
        torch.testing.assert_close(q.grad.cpu().double(), q64.grad, rtol=1e-3, atol=1e-3 * scale)
        torch.testing.assert_close(contrast.memory.cpu().double(), mem, rtol=0, atol=0)
        index = new_index
        assert contrast.index == index
    assert index < 2 * Bq                                                        # the ring pointer wrapped
    print(f"head D {D} K {K} Bq {Bq}: worst d q entry vs float64 {worst:.2e} of its largest entry")
    return worst


def check_e2e_head(tier, Bq, D):
    """mode 1 of the dense head (K = B, the ``grad_mem`` product): out = fk fq^T / T, NCESoftmaxLossNS, both gradients against
    float64 at the bars of the E2E head test (tests/test_wide_encoder_emu.py).  -> worst gradient error of its largest entry"""
    torch.manual_seed(3)
    fq0 = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1)
    fk0 = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1)
    fq, fk = tier.to(fq0).clone().requires_grad_(), tier.to(fk0).clone().requires_grad_()
    rq, rk = fq0.double().requires_grad_(), fk0.double().requires_grad_()
    out = e2e_logits(fq, fk, 0.07, engine=tier.wide_nce())
    loss = NCESoftmaxLossNS()(out)
    loss.backward()
    tier.sync()
    ref_out = rk @ rq.t() / 0.07                                                  # train.py:400
    ref_loss = E.nce_softmax_loss_ns(ref_out)
    ref_loss.backward()
    torch.testing.assert_close(out.dense().cpu().double(), ref_out.detach(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(loss.detach().cpu().double(), ref_loss.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out.prob.cpu().double().reshape(()), ref_out.diagonal().mean().detach(), rtol=1e-5, atol=1e-5)
    worst = max(float((a.grad.cpu().double() - b.grad).abs().max() / b.grad.abs().max()) for a, b in ((fq, rq), (fk, rk)))
    print(f"E2E head D {D} B {Bq}: worst gradient entry vs float64 {worst:.2e} of its largest entry")
    torch.testing.assert_close(fq.grad.cpu().double(), rq.grad, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(fk.grad.cpu().double(), rk.grad, rtol=1e-3, atol=1e-6)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# bf16 bodies: against tests/bf16_reference.py (the rule in float64 on the rounded values) under the Bars rule
def rounded_oracles(model, hidden, out, layers):
    """-> (the rounded oracle in fp32, the same in float64), both with the (CPU) model's state"""
    o32 = E.OracleGraphEncoder(node_hidden_dim=hidden, output_dim=out, num_layers=layers)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in o32.state_dict().items()}
    o32.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    R.round_gin_linears(o32)
    return o32, copy.deepcopy(o32).double()


def _run_oracle(o, args, keep, d, dt):
    o.zero_grad()
    feat, pooled = o(args[0], args[1], args[2], args[3].to(dt), dropout_masks=keep.to(dt), return_all_outputs=True)
    feat.backward(d.to(dt))
    return feat.detach(), [p.detach() for p in pooled], {n: p.grad for n, p in o.named_parameters()}


def check_bf16_against_rounded_oracle(model, o32, o64, q, keep, out, hidden, monkeypatch, nb=B, tier=EMU):
    """forward (features, pooled outputs), backward (every parameter gradient) and the running statistics of ONE training-mode
    pass of ``model`` on ``q`` against the rounded oracles -> (the oracle's arguments, Bars with the figures).  ``keep``: CPU"""
    keep_dev = tier.to(keep)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: keep_dev.clone())       # the API path draws its dropout masks here
    feat, pooled = model(q, return_all_outputs=True)
    assert tuple(feat.shape) == (nb, out) and all(tuple(t.shape) == (nb, hidden) for t in pooled)
    args = _oracle_args(q, nb)
    d = torch.randn(nb, out, generator=torch.Generator().manual_seed(out))
    f32, p32, g32 = _run_oracle(o32, args, keep, d, torch.float32)
    f64, p64, g64 = _run_oracle(o64, args, keep, d, torch.float64)
    feat.backward(tier.to(d))
    tier.sync()
    bars = Bars()
    bars.add("features", "feat", feat.detach(), f32, f64, rtol=2e-4, atol=2e-5)
    for i, (a, b32, b64) in enumerate(zip(pooled, p32, p64)):
        bars.add("pooled outputs", f"pooled[{i}]", a.detach(), b32, b64, rtol=2e-4, atol=2e-4)
    for name, p in model.named_parameters():
        if g64[name] is None:
            assert p.grad is None or float(p.grad.abs().sum()) == 0.0, name
            continue
        assert p.grad.shape == p.shape
        scale = max(float(g64[name].abs().max()), 1e-3)
        bars.add("gradients", f"d {name}", p.grad, g32[name], g64[name], rtol=0.0, atol=1e-3, unit=scale)
    s32, s64 = o32.state_dict(), o64.state_dict()       # running statistics moved as torch's BatchNorm1d moves them
    for k1, v1 in model.state_dict().items():
        if "running_" in k1:
            bars.add("running statistics", k1, v1, s32[k1], s64[k1], rtol=1e-4, atol=1e-5)
        elif "num_batches" in k1:
            assert torch.equal(v1.cpu(), s64[k1]), k1
    bars.check()
    return args, bars


def check_bf16_api_path(tier, hidden, out, layers, monkeypatch):
    """Forward features and pooled outputs, every parameter gradient, running statistics and eval mode against the rounded
    float64 oracle; d_in = 49 and the widths 72 / 96 / 40 / 80 leave partial k-tiles and edge tiles that are zero-filled in LDS.
    -> Bars of the training pass"""
    torch.manual_seed(hidden * 100 + out)
    model = encoder(hidden, out, layers, encoder_dtype="bf16")
    assert model.wide and not model.is_padded() and model.encoder_dtype == "bf16"
    o32, o64 = rounded_oracles(model, hidden, out, layers)
    model = tier.to(model)
    model._wide_engine = tier.wide_engine()
    model.train()
    o32.train()
    o64.train()
    q, _ = fixed_views(tier)
    keep = (torch.rand(layers, B, out, generator=torch.Generator().manual_seed(hidden)) >= 0.5).float()
    args, bars = check_bf16_against_rounded_oracle(model, o32, o64, q, keep, out, hidden, monkeypatch, tier=tier)
    print(f"{hidden}/{out}/{layers}: " + bars.summary())
    # the state survives a save / load round trip, and eval mode (running statistics, no dropout) agrees too
    m2 = encoder(hidden, out, layers, encoder_dtype="bf16")
    m2.load_state_dict({k: v.cpu().clone() for k, v in model.state_dict().items()})
    for o in (o32, o64):
        o.load_state_dict(m2.state_dict())        # (both oracles evaluate the SAME running statistics: the model's)
        o.eval()
    m2 = tier.to(m2)
    m2._wide_engine = tier.wide_engine()
    m2.eval()
    with torch.no_grad():
        e32 = o32(*args)
        e64 = o64(args[0], args[1], args[2], args[3].double())
        ev = Bars()
        ev.add("features", "eval feat", m2(q), e32, e64, rtol=2e-4, atol=2e-5)
        ev.add("features", "embed_views", m2.embed_views(q, q), e32, e64, rtol=2e-4, atol=2e-5)
        ev.check()
    assert_resolution(bars, f"{hidden}/{out}/{layers}")
    return bars


def _flag_runs(tier, monkeypatch):
    """-> {tag: {name: tensor}} of one training pass (features, pooled outputs, every gradient, running statistics) of three
    models with ONE state on the same inputs: built without the keyword, with encoder_dtype="f32", with "bf16" """
    hidden, out, layers = 96, 80, 3
    q, _ = fixed_views(tier)
    keep = tier.to((torch.rand(layers, B, out, generator=torch.Generator().manual_seed(1)) >= 0.5).float())
    monkeypatch.setattr(torch, "rand", lambda *a, **k: keep.clone())
    d = tier.to(torch.randn(B, out, generator=torch.Generator().manual_seed(2)))
    torch.manual_seed(5)
    plain = encoder(hidden, out, layers)
    res = {}
    for tag, kw in (("plain", {}), ("f32", dict(encoder_dtype="f32")), ("bf16", dict(encoder_dtype="bf16"))):
        m = encoder(hidden, out, layers, **kw)
        m.load_state_dict(plain.state_dict())
        m = tier.to(m)
        m._wide_engine = tier.wide_engine()
        m.train()
        p, _buf = m.wide_engine().make_pass(m, q, training=True, keep=keep)
        assert p.gemm_dtype == (1 if tag == "bf16" else 0)
        feat, pooled = m(q, return_all_outputs=True)
        feat.backward(d)
        tier.sync()
        res[tag] = dict([("feat", feat.detach())] + [(f"pooled[{i}]", t.detach()) for i, t in enumerate(pooled)]
                        + [(f"d {n}", p.grad) for n, p in m.named_parameters() if p.grad is not None]
                        + [(k, v) for k, v in m.state_dict().items() if "running_" in k])
    assert list(res["plain"]) == list(res["f32"]) == list(res["bf16"])
    return res


def _differing(a, b):
    """names of the tensors that are not bit-identical, with the largest difference in units of the tensor's largest entry"""
    return [f"{n}: {float((a[n] - b[n]).abs().max() / a[n].abs().max()):.1e} of its largest entry, {int((a[n] != b[n]).sum())} of "
            f"{a[n].numel()} entries" for n in a if not torch.equal(a[n], b[n])]


def check_bf16_flag(tier, monkeypatch):
    """bf16 and f32 mode differ on the same inputs; f32 mode is bit-identical to a model built without the keyword"""
    res = _flag_runs(tier, monkeypatch)
    assert not torch.equal(res["bf16"]["feat"], res["f32"]["feat"])
    assert len(_differing(res["bf16"], res["f32"])) > len(res["f32"]) // 2
    bad = _differing(res["plain"], res["f32"])
    assert not bad, "f32 mode is not bit-identical to a model built without the keyword: " + "; ".join(bad)


def check_f32_products_are_reproducible(tier, monkeypatch):
    """The part of the flag check that never went through an atomic reduction: the forward outputs, the running statistics and every
    Linear weight gradient (the GEMMs and their split-K slabs) of two models with one state are bit-identical.  A missing barrier
    or a cross-wave LDS reuse in a GEMM loop would show here as a difference between two runs."""
    res = _flag_runs(tier, monkeypatch)
    fixed = [n for n in res["plain"] if not n.startswith("d ") or ".linears." in n and n.endswith(".weight")
             or "linears_prediction" in n and n.endswith(".weight")]
    assert len(fixed) >= 15, fixed
    bad = _differing({n: res["plain"][n] for n in fixed}, res["f32"])
    assert not bad, "; ".join(bad)


def check_bf16_stale_rows(tier, n_live, monkeypatch):
    """node_cap 2,112; a 2,100-row batch goes through the same workspace slots first (forward and backward), so the rows past the
    live count hold its activations and gradients, and the dead input rows are NaN: the bf16 staging must never read them.  1,025
    and 2,049 live rows span two and three 1,024-row split-K slabs of the weight gradients (the last one a single row).  -> Bars"""
    hidden, out, layers, cap = 72, 72, 2, 2112
    torch.manual_seed(n_live)
    model = encoder(hidden, out, layers, encoder_dtype="bf16")
    o32, o64 = rounded_oracles(model, hidden, out, layers)
    model = tier.to(model)
    model._wide_engine = tier.wide_engine()
    model.train()
    big = hand_batch(2100, cap, 1, hub_degree=600, tier=tier)
    keep = masks(layers, out, 6)
    keep_dev = tier.to(keep)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: keep_dev.clone())
    for _ in range(2):                               # (the API path alternates between two slots: fill both)
        model(big).backward(tier.to(torch.ones(B, out)))
    model.zero_grad()
    for m in model.modules():                        # the oracles start from the state the checked pass starts from
        if isinstance(m, torch.nn.BatchNorm1d):
            m.reset_running_stats()
    o32.train()
    o64.train()
    g = hand_batch(n_live, cap, 10 + n_live, hub_degree=530, tier=tier)
    _, bars = check_bf16_against_rounded_oracle(model, o32, o64, g, keep, out, hidden, monkeypatch, nb=B, tier=tier)
    assert_resolution(bars, f"{n_live} live rows, bf16")
    return bars


def check_bf16_head(tier, D, K, Bq=40):
    """MemoryMoCo(inputSize > 64, nce_dtype="bf16"): dense logits, loss, prob and d loss / d q against the queue BEFORE the
    enqueue, under the rule in float64; the queue after the enqueue exactly; three steps with a wrapping ring pointer.
    -> Bars of the worst step (by d q error)"""
    torch.manual_seed(D + K)
    contrast = MemoryMoCo(D, None, K, 0.07, use_softmax=True, nce_dtype="bf16")
    assert contrast.wide
    mem = contrast.memory.clone()
    contrast = tier.to(contrast)
    contrast._engine = tier.wide_nce("bf16")
    index = K - 50 if K > 100 else 0
    if Bq < 40:
        index = K - Bq                                                           # (few rows per step: start at the ring's end)
    contrast.index = index
    kept = None
    for step in range(3):
        q0 = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1)
        k = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1)
        q = tier.to(q0).clone().requires_grad_()
        out = contrast(q, tier.to(k))
        loss = NCESoftmaxLoss()(out)
        loss.backward()
        tier.sync()
        r32 = R.moco_head(q0, k, mem, 0.07)
        r64 = R.moco_head(q0.double(), k.double(), mem.double(), 0.07)
        bars = Bars()                      # (the bars of tests/test_wide_encoder_emu.py's f32 head test)
        bars.add("logits", "out", out.dense(), r32["out"], r64["out"], rtol=1e-4, atol=1e-4)
        bars.add("logits", "out[:, 0]", out[:, 0], r32["out"][:, 0], r64["out"][:, 0], rtol=1e-4, atol=1e-4)
        bars.add("loss", "loss", loss.detach(), r32["loss"], r64["loss"], rtol=1e-5, atol=1e-6)
        bars.add("prob", "prob", out.prob, r32["prob"], r64["prob"], rtol=1e-5, atol=1e-5)
        bars.add("d q", "d q", q.grad, r32["grad_q"], r64["grad_q"], rtol=1e-3, atol=1e-3, unit=float(r64["grad_q"].abs().max()))
        bars.check()
        assert_resolution(bars, "", show=False)
        if kept is None or bars.worst("d q")[0] > kept.worst("d q")[0]:
            kept = bars
        ref_mem = mem.clone()
        ref_mem[(torch.arange(Bq) + index) % K] = k                             # memory_moco.py:55-61
        assert torch.equal(contrast.memory.cpu(), ref_mem)
        mem, index = ref_mem, (index + Bq) % K
        assert contrast.index == index
    assert index < 3 * Bq                                                        # the ring pointer wrapped
    assert_resolution(kept, f"bf16 head D {D} K {K} Bq {Bq}, worst of three steps")
    return kept


def check_bf16_e2e_head(tier, Bq=48, D=128):
    torch.manual_seed(3)
    fq0 = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1)
    fk0 = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1)
    fq, fk = tier.to(fq0).clone().requires_grad_(), tier.to(fk0).clone().requires_grad_()
    out = e2e_logits(fq, fk, 0.07, engine=tier.wide_nce("bf16"))
    loss = NCESoftmaxLossNS()(out)
    loss.backward()
    tier.sync()
    r32 = R.e2e_head(fq0, fk0, 0.07)
    r64 = R.e2e_head(fq0.double(), fk0.double(), 0.07)
    bars = Bars()
    bars.add("logits", "out", out.dense(), r32["out"], r64["out"], rtol=1e-4, atol=1e-4)
    bars.add("loss", "loss", loss.detach(), r32["loss"], r64["loss"], rtol=1e-5, atol=1e-6)
    bars.add("prob", "prob", out.prob, r32["prob"], r64["prob"], rtol=1e-5, atol=1e-5)
    for name, got in (("grad_q", fq.grad), ("grad_k", fk.grad)):
        bars.add("gradients", name, got, r32[name], r64[name], rtol=1e-3, atol=1e-3, unit=float(r64[name].abs().max()))
    bars.check()
    assert_resolution(bars, f"bf16 E2E head D {D} B {Bq}")
    return bars


def check_bf16_fused_step(tier):
    """MoCoTrainStep._body at hidden 128 with --encoder-dtype bf16 and --nce-dtype bf16, one step.  One GIN layer (num_layers
    2): every kind of bf16 product runs -- z1 with k = 49, z2, d a1, d agg, dW1 and dW0 over the node dimension, the head's three --
    while the rule's own fp32-vs-float64 gap stays near the f32 bars, so the comparison keeps its resolution (each further layer
    multiplies that gap: see the module docstring of tests/test_wide_bf16_emu.py).  -> Bars"""
    hidden, layers, K = 128, 2, 96
    tr, model, ema, contrast = fused_step(hidden, hidden, layers, [fixed_views(tier)], K=K, tier=tier, seed=128, nce_dtype="bf16",
                                          encoder_dtype="bf16")
    keep = tier.to((torch.rand(layers, B, hidden, generator=torch.Generator().manual_seed(4)) >= 0.5).float().contiguous())
    rep = check_wide_bf16_moco_step(tr, model, ema, contrast, 0.004, keep, sync=tier.sync, step_id=0)
    assert_resolution(rep["bars"], "fused bf16 step 128 / 2")
    return rep["bars"]
