"""``--encoder-dtype bf16`` / ``--nce-dtype bf16`` above 64 channels: the any-width encoder and the dense head of
gcc_amd/csrc/ginx.hip with bf16 operands on v_mfma_f32_16x16x32_bf16 (ginx_gemm_bf16_kernel; gcc_ginx_pass.gemm_dtype = 1,
gcc_ncex_forward_dt) against tests/bf16_reference.py -- the rule restated with plain torch and run in float64 on the rounded
values.  Emulator tier; the device tier is tests/test_wide_bf16_gpu.py.

Bars: those tests/test_wide_encoder_emu.py uses for the f32 mode -- features rtol 2e-4 / atol 2e-5 (pooled outputs atol 2e-4,
running statistics rtol 1e-4 / atol 1e-5), gradients 1e-3 of the tensor's largest entry against float64.  One thing is new in
this mode: an activation that differs by one fp32 ulp between two implementations can sit on a bf16 rounding boundary, and then
the two round it 2^-8 of its size apart.  That is a property of the rule, not of an implementation of it, so where it needs room
the room is MEASURED, never chosen: the same rounded oracle is run in fp32 and in float64 (two implementations of the rule,
neither the code under test) and a bar becomes max(its f32-mode value, twice that gap) -- :class:`Bars`.

The gap is taken per KIND of quantity, in the unit its bar is stated in: one figure for the features, one for the pooled outputs,
one for the running statistics, and for the gradients the worst entry of any tensor in units of that tensor's largest entry.
Which activations tip is decided by the last bit of an fp32 sum, and one tip moves everything downstream of it by an amount that
depends on where it happened to fall (measured at 256 / 256 / 5: torch's fp32 run and the kernels each tip 4 of the 144,128
activations behind the first BatchNorm -- different ones; torch's move the next pooled output by 9.9e-4, the kernels' by 3.6e-3;
two layers on both have tipped ~15 % of all activations).  The gap of ONE tensor is a single draw of that lottery; the worst over
the tensors of a kind is what the rule needs.  Every comparison prints its figures before it is asserted.

Measured here (emulator; err = this code, gap = the rounded oracle's fp32 run, both against its float64 run; gradients in units
of the tensor's largest entry):
    widths / layers   features err | gap      pooled err | gap        gradients err | gap     running statistics err | gap
    128 / 128 / 5     1.3e-4 | 6.3e-4         4.8e-2 | 2.0e-1         3.0e-2 | 1.3e-1         2.9e-4 | 3.2e-3
    96 / 80 / 3       1.6e-7 | 3.2e-7         1.0e-5 | 5.2e-5         8.2e-4 | 1.3e-3         5.1e-7 | 5.1e-7
    256 / 256 / 5     3.8e-4 | 3.2e-4         4.2e-1 | 4.5e-1         7.1e-2 | 6.8e-2         3.5e-3 | 3.1e-3
    72 / 40 / 2       2.9e-7 | 2.8e-7         4.9e-5 | 4.8e-5         3.0e-4 | 1.5e-3         6.0e-8 | 6.9e-8
    fused step, 128 / 2 layers: embeddings 7.2e-6 | 6.9e-7, gradients 2.3e-4 | 1.9e-4 (inside the f32 bars)
    head (D, K) = (128, 96), (80, 200), (96, 4400), E2E: logits <= 1.5e-6 | 1.5e-6, d q <= 3.8e-6 | 5.0e-7 of its largest entry
Up to three layers the kernels follow the rule to fp32 rounding; at five the rule itself is conditioned as the gap column says.
"""
import copy
import ctypes

import pytest
import torch

from gcc_amd import _cabi
from gcc_amd.contrast import MemoryMoCo, NCESoftmaxLoss, NCESoftmaxLossNS, WideNceEngine, e2e_logits
from gcc_amd.encoder import GraphEncoder
from gcc_amd.train_step import MoCoTrainStep
from oracle import encoder as E
from tests import bf16_reference as R
from tests.hipemu.emu_driver import emu_lib
from tests.test_headline_step_emu import B
from tests.test_nce_emu import emu_nce
from tests.test_wide_edges_emu import B as HB
from tests.test_wide_edges_emu import _masks, hand_batch
from tests.test_wide_encoder_emu import emu_wide_engine, fixed_views
from tests.wide_bf16_step_check import Bars, check_wide_bf16_moco_step


def wide_encoder(hidden, out, layers=5, **kw):
    return GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=512,
                        freq_embedding_size=16, degree_embedding_size=16, output_dim=out, node_hidden_dim=hidden,
                        edge_hidden_dim=hidden, num_layers=layers, num_step_set2set=6, num_layer_set2set=3, norm=True,
                        gnn_model="gin", degree_input=True, **kw)


def emu_wide_nce(dtype="bf16"):
    return WideNceEngine(lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr(), dtype=dtype)


def _keep(layers, nb, out, seed):
    return (torch.rand(layers, nb, out, generator=torch.Generator().manual_seed(seed)) >= 0.5).float()


def _rounded_oracles(model, hidden, out, layers):
    """-> (the rounded oracle in fp32, the same in float64), both with the model's state"""
    o32 = E.OracleGraphEncoder(node_hidden_dim=hidden, output_dim=out, num_layers=layers)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in o32.state_dict().items()}
    o32.load_state_dict(model.state_dict())
    R.round_gin_linears(o32)
    return o32, copy.deepcopy(o32).double()


def _run_oracle(o, args, keep, d, dt):
    o.zero_grad()
    feat, pooled = o(args[0], args[1], args[2], args[3].to(dt), dropout_masks=keep.to(dt), return_all_outputs=True)
    feat.backward(d.to(dt))
    return feat.detach(), [p.detach() for p in pooled], {n: p.grad for n, p in o.named_parameters()}


def check_bf16_against_rounded_oracle(model, o32, o64, q, keep, out, hidden, monkeypatch, nb=B):
    """forward (features, pooled outputs), backward (every parameter gradient) and the running statistics of ONE training-mode
    pass of ``model`` on ``q`` against the rounded oracles -> (the oracle's arguments, Bars with the figures)"""
    monkeypatch.setattr(torch, "rand", lambda *a, **k: keep.clone())       # the API path draws its dropout masks here
    feat, pooled = model(q, return_all_outputs=True)
    assert tuple(feat.shape) == (nb, out) and all(tuple(t.shape) == (nb, hidden) for t in pooled)
    n = int(q.node_off[nb])
    args = (q.node_off.long(), q.row_ptr[: n + 1].long(), q.col_idx.long(), q.pos_undirected[:n])
    d = torch.randn(nb, out, generator=torch.Generator().manual_seed(out))
    f32, p32, g32 = _run_oracle(o32, args, keep, d, torch.float32)
    f64, p64, g64 = _run_oracle(o64, args, keep, d, torch.float64)
    feat.backward(d)
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
            assert torch.equal(v1, s64[k1]), k1
    bars.check()
    return args, bars


@pytest.mark.parametrize("hidden,out,layers", [(128, 128, 5), (96, 80, 3), (256, 256, 5), (72, 40, 2)])
def test_bf16_api_path_forward_backward_vs_rounded_oracle(hidden, out, layers, monkeypatch):
    """Forward features and pooled outputs, every parameter gradient, running statistics and eval mode against the rounded
    float64 oracle; d_in = 49 and the widths 72 / 96 / 40 / 80 leave partial k-tiles and edge tiles that are zero-filled in LDS."""
    torch.manual_seed(hidden * 100 + out)
    model = wide_encoder(hidden, out, layers, encoder_dtype="bf16")
    assert model.wide and not model.is_padded() and model.encoder_dtype == "bf16"
    o32, o64 = _rounded_oracles(model, hidden, out, layers)
    model._wide_engine = emu_wide_engine()
    model.train()
    o32.train()
    o64.train()
    q, _ = fixed_views()
    args, bars = check_bf16_against_rounded_oracle(model, o32, o64, q, _keep(layers, B, out, hidden), out, hidden, monkeypatch)
    print(f"{hidden}/{out}/{layers}: " + bars.summary())
    # the state survives a save / load round trip, and eval mode (running statistics, no dropout) agrees too
    m2 = wide_encoder(hidden, out, layers, encoder_dtype="bf16")
    m2.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    m2._wide_engine = emu_wide_engine()
    m2.eval()
    for o in (o32, o64):
        o.load_state_dict(m2.state_dict())        # (both oracles evaluate the SAME running statistics: the model's)
        o.eval()
    with torch.no_grad():
        e32 = o32(*args)
        e64 = o64(args[0], args[1], args[2], args[3].double())
        ev = Bars()
        ev.add("features", "eval feat", m2(q), e32, e64, rtol=2e-4, atol=2e-5)
        ev.add("features", "embed_views", m2.embed_views(q, q), e32, e64, rtol=2e-4, atol=2e-5)
        ev.check()


def test_the_flag_does_something_and_f32_mode_is_untouched(monkeypatch):
    """bf16 and f32 mode differ on the same inputs; f32 mode is bit-identical to a model built without the keyword"""
    hidden, out, layers = 96, 80, 3
    q, _ = fixed_views()
    keep = _keep(layers, B, out, 1)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: keep.clone())
    d = torch.randn(B, out, generator=torch.Generator().manual_seed(2))
    torch.manual_seed(5)
    plain = wide_encoder(hidden, out, layers)
    res = {}
    for tag, kw in (("plain", {}), ("f32", dict(encoder_dtype="f32")), ("bf16", dict(encoder_dtype="bf16"))):
        m = wide_encoder(hidden, out, layers, **kw)
        m.load_state_dict(plain.state_dict())
        m._wide_engine = emu_wide_engine()
        m.train()
        p, _buf = m.wide_engine().make_pass(m, q, training=True, keep=keep)
        assert p.gemm_dtype == (1 if tag == "bf16" else 0)
        feat, pooled = m(q, return_all_outputs=True)
        feat.backward(d)
        res[tag] = [feat.detach()] + [t.detach() for t in pooled] + [p.grad for p in m.parameters() if p.grad is not None] \
            + [v for k, v in m.state_dict().items() if "running_" in k]
    assert len(res["plain"]) == len(res["f32"]) == len(res["bf16"])
    for a, b in zip(res["plain"], res["f32"]):
        assert torch.equal(a, b)
    assert not torch.equal(res["bf16"][0], res["f32"][0])
    assert sum(not torch.equal(a, b) for a, b in zip(res["bf16"], res["f32"])) > len(res["f32"]) // 2


@pytest.mark.parametrize("n_live", [1023, 1025, 2049])
def test_bf16_on_hand_built_batches_over_stale_rows(n_live, monkeypatch):
    """node_cap 2,112; a 2,100-row batch goes through the same workspace slots first (forward and backward), so the rows past the
    live count hold its activations and gradients, and the dead input rows are NaN: the bf16 staging must never read them.  1,025
    and 2,049 live rows span two and three 1,024-row split-K slabs of the weight gradients (the last one a single row)."""
    hidden, out, layers, cap = 72, 72, 2, 2112
    torch.manual_seed(n_live)
    model = wide_encoder(hidden, out, layers, encoder_dtype="bf16")
    o32, o64 = _rounded_oracles(model, hidden, out, layers)
    model._wide_engine = emu_wide_engine()
    model.train()
    big = hand_batch(2100, cap, 1, hub_degree=600)
    keep = _masks(layers, out, 6)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: keep.clone())
    for _ in range(2):                               # (the API path alternates between two slots: fill both)
        model(big).backward(torch.ones(HB, out))
    model.zero_grad()
    for m in model.modules():                        # the oracles start from the state the checked pass starts from
        if isinstance(m, torch.nn.BatchNorm1d):
            m.reset_running_stats()
    o32.train()
    o64.train()
    g = hand_batch(n_live, cap, 10 + n_live, hub_degree=530)
    check_bf16_against_rounded_oracle(model, o32, o64, g, keep, out, hidden, monkeypatch, nb=HB)


@pytest.mark.parametrize("D,K", [(128, 96), (80, 200), (96, 4400)])    # (K >= 4096: the split reduction of d loss / d q)
def test_bf16_wide_moco_head_vs_rounded_reference(D, K):
    """MemoryMoCo(inputSize > 64, nce_dtype="bf16"): dense logits, loss, prob and d loss / d q against the queue BEFORE the
    enqueue, under the rule in float64; the queue after the enqueue exactly; three steps with a wrapping ring pointer."""
    torch.manual_seed(D + K)
    Bq = 40
    contrast = MemoryMoCo(D, None, K, 0.07, use_softmax=True, nce_dtype="bf16")
    assert contrast.wide
    contrast._engine = emu_wide_nce()
    mem = contrast.memory.clone()
    index = K - 50 if K > 100 else 0
    contrast.index = index
    for step in range(3):
        q = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1).requires_grad_()
        k = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1)
        out = contrast(q, k)
        loss = NCESoftmaxLoss()(out)
        loss.backward()
        r32 = R.moco_head(q.detach(), k, mem, 0.07)
        r64 = R.moco_head(q.detach().double(), k.double(), mem.double(), 0.07)
        bars = Bars()                      # (the bars of tests/test_wide_encoder_emu.py's f32 head test)
        bars.add("logits", "out", out.dense(), r32["out"], r64["out"], rtol=1e-4, atol=1e-4)
        bars.add("logits", "out[:, 0]", out[:, 0], r32["out"][:, 0], r64["out"][:, 0], rtol=1e-4, atol=1e-4)
        bars.add("loss", "loss", loss.detach(), r32["loss"], r64["loss"], rtol=1e-5, atol=1e-6)
        bars.add("prob", "prob", out.prob, r32["prob"], r64["prob"], rtol=1e-5, atol=1e-5)
        bars.add("d q", "d q", q.grad, r32["grad_q"], r64["grad_q"], rtol=1e-3, atol=1e-3, unit=float(r64["grad_q"].abs().max()))
        bars.check()
        ref_mem = mem.clone()
        ref_mem[(torch.arange(Bq) + index) % K] = k                             # memory_moco.py:55-61
        assert torch.equal(contrast.memory, ref_mem)
        mem, index = ref_mem, (index + Bq) % K
        assert contrast.index == index
    assert index < 3 * Bq                                                        # the ring pointer wrapped


def test_bf16_wide_head_differs_from_f32_head():
    torch.manual_seed(1)
    q = torch.nn.functional.normalize(torch.randn(40, 128), dim=1)
    k = torch.nn.functional.normalize(torch.randn(40, 128), dim=1)
    mem = torch.nn.functional.normalize(torch.randn(96, 128), dim=1)
    a = emu_wide_nce("f32").forward(q, k, mem, 0.07, 0)
    b = emu_wide_nce("bf16").forward(q, k, mem, 0.07, 0)
    assert torch.equal(a["out"][:, 0], b["out"][:, 0])                          # the positive logit stays f32
    assert not torch.equal(a["out"], b["out"]) and not torch.equal(a["grad_rows"], b["grad_rows"])


def test_bf16_wide_e2e_head_vs_rounded_reference():
    torch.manual_seed(3)
    Bq, D = 48, 128
    fq = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1).requires_grad_()
    fk = torch.nn.functional.normalize(torch.randn(Bq, D), dim=1).requires_grad_()
    out = e2e_logits(fq, fk, 0.07, engine=emu_wide_nce())
    loss = NCESoftmaxLossNS()(out)
    loss.backward()
    r32 = R.e2e_head(fq.detach(), fk.detach(), 0.07)
    r64 = R.e2e_head(fq.detach().double(), fk.detach().double(), 0.07)
    bars = Bars()
    bars.add("logits", "out", out.dense(), r32["out"], r64["out"], rtol=1e-4, atol=1e-4)
    bars.add("loss", "loss", loss.detach(), r32["loss"], r64["loss"], rtol=1e-5, atol=1e-6)
    bars.add("prob", "prob", out.prob, r32["prob"], r64["prob"], rtol=1e-5, atol=1e-5)
    for name, got in (("grad_q", fq.grad), ("grad_k", fk.grad)):
        bars.add("gradients", name, got, r32[name], r64[name], rtol=1e-3, atol=1e-3, unit=float(r64[name].abs().max()))
    bars.check()


def test_fused_wide_step_bf16_encoder_and_head_vs_rounded_oracle():
    """MoCoTrainStep._body at hidden 128 with --encoder-dtype bf16 and --nce-dtype bf16, one step.  One GIN layer (num_layers
    2): every kind of bf16 product runs -- z1 with k = 49, z2, d a1, d agg, dW1 and dW0 over the node dimension, the head's three --
    while the rule's own fp32-vs-float64 gap stays near the f32 bars, so the comparison keeps its resolution (each further layer
    multiplies that gap: see the module docstring)."""
    hidden, layers, K = 128, 2, 96
    torch.manual_seed(128)
    model, ema = wide_encoder(hidden, hidden, layers, encoder_dtype="bf16"), wide_encoder(hidden, hidden, layers, encoder_dtype="bf16")
    ema.load_state_dict(model.state_dict())
    model._wide_engine = ema._wide_engine = emu_wide_engine()
    contrast = MemoryMoCo(hidden, None, K, 0.07, use_softmax=True, nce_dtype="bf16")
    contrast._engine = emu_wide_nce()

    class _Views:
        batch_size = B

        def sample(self, first_id, prof=None):
            return fixed_views()

    tr = MoCoTrainStep(model, ema, contrast, _Views(), posemb=lambda gr: gr, prefetch=False, flat_engine=emu_nce())
    assert tr.wide and not tr.use_graph and tr.nce.dtype == "bf16"
    masks = (torch.rand(layers, B, hidden, generator=torch.Generator().manual_seed(4)) >= 0.5).float().contiguous()
    rep = check_wide_bf16_moco_step(tr, model, ema, contrast, 0.004, masks, step_id=0)
    print("fused bf16 step: " + rep["bars"].summary())


def test_refusals():
    with pytest.raises(NotImplementedError, match="compute in f32"):
        wide_encoder(64, 64, 5, encoder_dtype="bf16")
    with pytest.raises(NotImplementedError, match="compute in f32"):
        GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=512, freq_embedding_size=16,
                     degree_embedding_size=16, output_dim=64, node_hidden_dim=64, edge_hidden_dim=64, num_layers=2, norm=True,
                     gnn_model="gat", degree_input=True, encoder_dtype="bf16")
    with pytest.raises(ValueError, match="encoder_dtype"):
        wide_encoder(128, 128, 5, encoder_dtype="fp8")
    # the C ABI refuses gemm_dtype = 2, in the encoder pass and in the head
    model = wide_encoder(72, 40, 2)
    eng = emu_wide_engine()
    q, _ = fixed_views()
    p, _buf = eng.make_pass(model, q, training=True)
    p.gemm_dtype = 2
    with pytest.raises(RuntimeError, match="gemm_dtype 2"):
        eng.forward(p)
    grads = _cabi.GccGinGrads()
    assert eng.lib.gcc_ginx_backward(ctypes.byref(p), 1, ctypes.byref(grads), None) != 0
    assert b"gemm_dtype 2" in eng.lib.gcc_last_error()
    nce = emu_wide_nce()
    o = dict(t=torch.zeros(8, 200))
    ptr = o["t"].data_ptr()
    rc = nce.lib.gcc_ncex_forward_dt(ptr, ptr, ptr, 2, 4, 72, 1.0, 0, ptr, ptr, ptr, None, ptr, ptr, ptr, 2, None)
    assert rc != 0 and b"gemm_dtype 2" in nce.lib.gcc_last_error()
    with pytest.raises(ValueError, match="nce_dtype"):
        MemoryMoCo(128, None, 96, 0.07, use_softmax=True, nce_dtype="fp8")
