"""Shared body of the fused any-width step checks: ONE ``MoCoTrainStep.step`` at --hidden-size above 64 (``_body`` on csrc/ginx.hip
forward of both views, the dense head, the backward, clip + Adam + EMA + meters, the enqueue) against oracle/encoder.py built with
the model's own widths, layer count and degree table, fed the same batch, dropout masks, weights, Adam moments and queue -- in fp32
and in float64.  Used by both tiers at the edges (tests/wide_edges_check.py) and by the device tier on a sampled batch
(tests/test_wide_step_gpu.py).  TEST INFRASTRUCTURE ONLY.

The bar for gradients is north_star's: 1e-3 of the tensor's largest entry against the float64 run, with no allowance for fp32
(a weight gradient sums thousands of terms that largely cancel; the kernels accumulate those sums in fp64).  The one exception is
the bias of a Linear in front of a BatchNorm, whose exact gradient is zero: there both sides are rounding noise and the bar is
1e-4 absolute, as in tests/headline_step_check.py."""
import torch

from gcc_amd.encoder import grad_params
from oracle import encoder as E
from tests.headline_step_check import _seed_adam, _state, view_arrays


def oracle_like(model, dtype=torch.float32, state=None):
    """oracle/encoder.py with ``model``'s widths, depth and degree table, loaded with ``state`` (default: the model's current one)"""
    om = E.OracleGraphEncoder(positional_embedding_size=model.positional_embedding_size, max_degree=model.max_degree,
                              degree_embedding_size=model.degree_embedding_size, output_dim=model.output_dim,
                              node_hidden_dim=model.hidden, num_layers=len(model.gnn.ginlayers) + 1, norm=model.norm)
    om.load_state_dict({k: v.detach().cpu().clone() for k, v in (state if state is not None else model.state_dict()).items()})
    if dtype == torch.float64:
        om = om.double()
    return om


def grad_bar(name, g64):
    """(scale, absolute tolerance = 1e-3 * scale) of a gradient tensor against its float64 value: the scale is the tensor's
    largest entry, at least 1e-3 (0.1 where the exact gradient is zero and both sides are rounding noise)"""
    noise = 1e-4 if (".mlp.linears." in name and name.endswith(".bias")) else 0.0
    scale = max(float(g64.abs().max()), 1e-3, 1e3 * noise)
    return scale, 1e-3 * scale


def check_wide_moco_step(tr, model, ema, contrast, lr, masks, sync=lambda: None, step_id=0, rtol=1e-3):
    """``masks``: float keep masks [L + 1, B, output_dim] on the trainer's device.  Returns a report dict; its
    ``grad_err_vs_f64_step`` / ``grad_err_vs_f64_torch32`` are the worst gradient entries of the step and of torch's fp32 run of
    the oracle against float64, in units of the tensor's largest entry."""
    assert tr.wide and model.wide and ema.wide
    L = len(model.gnn.ginlayers)
    assert tuple(masks.shape) == (L + 1, tr.B, model.output_dim), tuple(masks.shape)
    init_m, init_e = _state(model), _state(ema)
    adam0 = (tr.optimizer.exp_avg.detach().cpu().clone(), tr.optimizer.exp_avg_sq.detach().cpu().clone(), int(tr.optimizer.steps))
    mem0 = contrast.memory.detach().cpu().clone()
    index0, K, B, T, alpha = int(contrast.index), contrast.queueSize, tr.B, contrast.T, tr.alpha
    tr.mask_fn = lambda: masks
    out = tr.step(step_id, lr)
    sync()
    gq, gk = out["graph_q"], out["graph_k"]
    (aq, pos_q), (ak, pos_k) = view_arrays(gq), view_arrays(gk)
    report = dict(batch_size=B, K=K, hidden=model.hidden, out_dim=model.output_dim, layers=L + 1,
                  nodes_q=int(aq[0][-1]), nodes_k=int(ak[0][-1]), edges_q=len(aq[2]), edges_k=len(ak[2]))
    omask = masks.detach().cpu()
    # ---- the oracle in fp32 (torch's own arithmetic) and in float64 (exact for this purpose)
    runs = {}
    for dt in (torch.float32, torch.float64):
        om, oe = oracle_like(model, dt, init_m), oracle_like(ema, dt, init_e)
        om.train()
        oe.train()                                   # train.py:357-365: eval() + BatchNorm back to train(); dropout stays off
        rq = om(*aq, pos_q.to(dt), dropout_masks=omask.to(dt))
        with torch.no_grad():
            rk = oe(*ak, pos_k.to(dt))
        mem = mem0.to(dt, copy=True)
        rout, ref_index = E.moco_forward(mem, index0, rq, rk, T)
        rloss = E.nce_softmax_loss(rout)
        opt = torch.optim.Adam(om.parameters(), lr=lr, betas=(0.9, 0.999), weight_decay=1e-5)   # train.py:667-672
        _seed_adam(opt, om, model, tr, *(t.to(dt) if torch.is_tensor(t) else t for t in adam0))
        opt.zero_grad()
        rloss.backward()
        grads = {n: p.grad.detach().clone() for n, p in om.named_parameters() if p.grad is not None}
        rgn = torch.nn.utils.clip_grad_norm_(om.parameters(), tr.clip_norm)                    # train.py:409
        opt.step()
        E.moment_update(om, oe, alpha)                                                          # train.py:430-431
        runs[dt] = dict(q=rq.detach(), k=rk.detach(), loss=rloss.detach(), prob=rout[:, 0].mean().detach(), grads=grads,
                        gn=float(rgn), mem=mem, index=ref_index, m=om.state_dict(), e=oe.state_dict())
    r32, r64 = runs[torch.float32], runs[torch.float64]
    # ---- embeddings, loss, prob, gradient norm
    feat_q, feat_k = tr.last_bufs[0]["feat"].detach().cpu(), tr.last_bufs[1]["feat"].detach().cpu()
    torch.testing.assert_close(feat_q.double(), r64["q"], rtol=rtol, atol=1e-4, msg=lambda m: f"feat_q: {m}")
    torch.testing.assert_close(feat_k.double(), r64["k"], rtol=rtol, atol=1e-4, msg=lambda m: f"feat_k: {m}")
    loss, prob = out["loss"].reshape(()).cpu().double(), out["prob"].reshape(()).cpu().double()
    torch.testing.assert_close(loss, r64["loss"], rtol=rtol, atol=1e-5, msg=lambda m: f"loss: {m}")
    torch.testing.assert_close(prob, r64["prob"], rtol=rtol, atol=1e-5, msg=lambda m: f"prob: {m}")
    gn = float(torch.as_tensor(out["grad_norm"]).reshape(()))
    assert abs(gn - r64["gn"]) <= rtol * r64["gn"] + 1e-6, f"grad_norm {gn} vs float64 oracle {r64['gn']}"
    report.update(loss=float(loss), loss_f64=float(r64["loss"]), prob=float(prob), grad_norm=gn, grad_norm_f64=r64["gn"],
                  grad_norm_torch32=r32["gn"], feat_q_max_abs_err=float((feat_q.double() - r64["q"]).abs().max()),
                  feat_k_max_abs_err=float((feat_k.double() - r64["k"]).abs().max()))
    # ---- every gradient (the flat buffer is clipped in place, as clip_grad_norm_ clips .grad) against float64
    coef = min(1.0, tr.clip_norm / (gn + 1e-6)) if tr.clip_norm > 0 else 1.0        # (the step clips by the norm it computed)
    names = {id(p): n for n, p in model.named_parameters()}
    flat = tr.flat_grad.detach().cpu()
    off, w_step, w_t32, worst_name, by_tensor = 0, 0.0, 0.0, None, {}
    for _, _, p in grad_params(model):
        n = names[id(p)]
        got = flat[off:off + p.numel()].view_as(p).double() / coef
        off += p.numel()
        g64 = r64["grads"][n]
        scale, atol = grad_bar(n, g64)
        err = float((got - g64).abs().max())
        assert err <= atol, f"d {n}: {err:.3e} from the float64 oracle (bar {atol:.3e}, tensor scale {scale:.3e})"
        e32 = float((r32["grads"][n].double() - g64).abs().max()) / scale
        by_tensor[n] = (err / scale, e32)
        if err / scale > w_step:
            w_step, worst_name = err / scale, n
        w_t32 = max(w_t32, e32)
    assert off == tr.n_live
    report.update(grad_err_vs_f64_step=w_step, grad_err_vs_f64_torch32=w_t32, grad_worst_tensor=worst_name,
                  grad_err_by_tensor=by_tensor)
    # ---- Adam: every weight within 2.1 lr of the float64 oracle's (check_moco_step's bar: a first Adam step moves a weight by
    # ~lr * sign(g), and where a gradient entry is rounding noise its sign is no reference), and the update itself exactly as
    # torch.optim.Adam makes it from the step's own clipped gradient (checked above) and moments, recomputed in float64
    after_m, after_e = _state(model), _state(ema)
    grp = tr.optimizer.param_groups[0]
    (b1, b2), eps, wd, t = grp["betas"], grp["eps"], grp["weight_decay"], adam0[2] + 1
    off = 0
    for _, _, p in grad_params(model):
        n = names[id(p)]
        sl = slice(off, off + p.numel())
        off += p.numel()
        p0 = init_m[n].double().reshape(-1)
        g = flat[sl].double() + wd * p0
        m = b1 * adam0[0][sl].double() + (1 - b1) * g
        v = b2 * adam0[1][sl].double() + (1 - b2) * g * g
        want = p0 - lr * (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps)
        torch.testing.assert_close(after_m[n].double().reshape(-1), want, rtol=1e-5, atol=1e-6, msg=lambda msg, n=n: f"Adam update of {n}: {msg}")
    for k, v in after_m.items():                      # weights vs float64 oracle; running statistics; num_batches_tracked
        ref = r64["m"][k]
        if not v.dtype.is_floating_point:
            assert torch.equal(v, ref), k
        elif "running_" in k:
            torch.testing.assert_close(v.double(), ref, rtol=rtol, atol=1e-5, msg=lambda m, k=k: f"model {k}: {m}")
        else:
            torch.testing.assert_close(v.double(), ref, rtol=5e-3, atol=2.1 * lr, msg=lambda m, k=k: f"model {k}: {m}")
    for k, v in after_e.items():
        ref = r64["e"][k]
        if v.dtype.is_floating_point:
            torch.testing.assert_close(v.double(), ref, rtol=rtol, atol=2e-5, msg=lambda m, k=k: f"model_ema {k}: {m}")
        else:
            assert torch.equal(v, ref), k
    # ---- queue: rows [index0, index0 + B) are the keys, every other row untouched (memory_moco.py:55-61)
    mem = contrast.memory.detach().cpu()
    torch.testing.assert_close(mem.double(), r64["mem"], rtol=rtol, atol=1e-4, msg=lambda m: f"queue: {m}")
    ids = (torch.arange(B) + index0) % K
    rest = torch.ones(K, dtype=torch.bool)
    rest[ids] = False
    assert torch.equal(mem[rest], mem0[rest])
    assert int(contrast.index) == r64["index"]
    return report
