"""tests/wide_step_check.py for ``--encoder-dtype bf16 --nce-dtype bf16``: ONE ``MoCoTrainStep.step`` of the any-width step
(``_body`` on the any-width engines) whose per-node Linears and dense head run with bf16 operands, against the ROUNDED oracle of
tests/bf16_reference.py -- oracle/encoder.py with the GIN layers' Linears swapped for the rule's, and the head's three products
under the rule -- fed the same batch, dropout masks, weights, Adam moments and queue, in fp32 and in float64.  The float64 run
on the rounded values is the exact value of the rule; the fp32 run is a second implementation of it, and its distance from the
float64 run is the room an activation on a bf16 rounding boundary needs (tests/test_wide_bf16_emu.py).  Used by the emulator tier
and by the device tier (tests/test_wide_bf16_gpu.py).  TEST INFRASTRUCTURE ONLY.

Bars: tests/wide_step_check.py's -- gradients 1e-3 of the tensor's largest entry against float64 (1e-4 absolute for a Linear bias
in front of a BatchNorm, whose exact gradient is zero), embeddings / loss / prob / gradient norm 1e-3 relative -- each widened,
where the rule itself needs it, to twice the measured fp32-vs-float64 gap of the rounded oracle (:class:`Bars`)."""
import torch

from gcc_amd.encoder import grad_params
from oracle import encoder as E
from tests import bf16_reference as R
from tests.headline_step_check import _seed_adam, _state, view_arrays
from tests.wide_step_check import grad_bar, oracle_like


class Bars:
    """Comparisons against the rule's float64 run whose absolute bars are max(the f32 mode's bar, twice the MEASURED gap between the
    rule's fp32 and float64 runs).  The gap is taken per ``kind`` of quantity (features, pooled outputs, gradients, ...): the
    largest, over the comparisons of that kind, of max |fp32 run - float64 run| in the comparison's ``unit`` (1, or the tensor's
    largest entry where the bar is stated relative to it).  :meth:`add` records, :meth:`check` prints every figure and asserts."""

    def __init__(self):
        self.rows = []

    def add(self, kind, what, got, a32, a64, rtol, atol, unit=1.0):
        got, a32, a64 = (torch.as_tensor(t).detach().double().cpu() for t in (got, a32, a64))
        err = (got - a64).abs()
        self.rows.append(dict(kind=kind, what=what, unit=unit, atol=atol, rtol=rtol, err=float(err.max()) / unit,
                              excess=float((err - rtol * a64.abs()).max()) / unit, gap=float((a32 - a64).abs().max()) / unit))

    def gap(self, kind):
        return max(r["gap"] for r in self.rows if r["kind"] == kind)

    def bar(self, row):
        return max(row["atol"], 2.0 * self.gap(row["kind"]))

    def worst(self, kind):
        """(largest error, the kind's gap), both in the kind's unit"""
        return max(r["err"] for r in self.rows if r["kind"] == kind), self.gap(kind)

    def summary(self):
        kinds = list(dict.fromkeys(r["kind"] for r in self.rows))
        return "; ".join("%s err %.2e | rule gap %.2e" % ((k,) + self.worst(k)) for k in kinds)

    def check(self):
        for r in self.rows:
            print(f"{r['what']}: err {r['err']:.3e}, rule fp32-vs-float64 gap {r['gap']:.3e} ({r['kind']}: {self.gap(r['kind']):.3e}), "
                  f"bar {self.bar(r):.3e}" + (f" of {r['unit']:.3e}" if r["unit"] != 1.0 else "") + (f" + {r['rtol']} relative" if r["rtol"] else ""))
        bad = [r for r in self.rows if not r["excess"] <= self.bar(r)]
        assert not bad, "; ".join(f"{r['what']}: {r['err']:.3e} from the rounded float64 oracle, bar {self.bar(r):.3e}"
                                  + (f" of {r['unit']:.3e}" if r["unit"] != 1.0 else "") for r in bad)


def check_wide_bf16_moco_step(tr, model, ema, contrast, lr, masks, sync=lambda: None, step_id=0, rtol=1e-3):
    """``masks``: float keep masks [L + 1, B, output_dim] on the trainer's device.  Returns a report dict; ``bars`` holds every
    figure (:meth:`Bars.summary`)."""
    assert tr.wide and model.wide and ema.wide
    assert model.encoder_dtype == ema.encoder_dtype == "bf16" and contrast.nce_dtype == "bf16"
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
    runs = {}
    for dt in (torch.float32, torch.float64):
        om, oe = R.round_gin_linears(oracle_like(model, dt, init_m)), R.round_gin_linears(oracle_like(ema, dt, init_e))
        om.train()
        oe.train()                                   # train.py:357-365: eval() + BatchNorm back to train(); dropout stays off
        rq = om(*aq, pos_q.to(dt), dropout_masks=omask.to(dt))
        with torch.no_grad():
            rk = oe(*ak, pos_k.to(dt))
        mem = mem0.to(dt, copy=True)
        head = R.moco_head(rq.detach(), rk, mem, T)                              # against the queue BEFORE the enqueue
        opt = torch.optim.Adam(om.parameters(), lr=lr, betas=(0.9, 0.999), weight_decay=1e-5)   # train.py:667-672
        _seed_adam(opt, om, model, tr, *(t.to(dt) if torch.is_tensor(t) else t for t in adam0))
        opt.zero_grad()
        rq.backward(head["grad_q"])
        grads = {n: p.grad.detach().clone() for n, p in om.named_parameters() if p.grad is not None}
        rgn = torch.nn.utils.clip_grad_norm_(om.parameters(), tr.clip_norm)                    # train.py:409
        opt.step()
        E.moment_update(om, oe, alpha)                                                          # train.py:430-431
        runs[dt] = dict(q=rq.detach(), k=rk.detach(), loss=head["loss"], prob=head["prob"], grads=grads, gn=float(rgn),
                        m=om.state_dict(), e=oe.state_dict())
    r32, r64 = runs[torch.float32], runs[torch.float64]
    bars = Bars()
    feat_q, feat_k = tr.last_bufs[0]["feat"].detach().cpu(), tr.last_bufs[1]["feat"].detach().cpu()
    bars.add("embeddings", "feat_q", feat_q, r32["q"], r64["q"], rtol=rtol, atol=1e-4)
    bars.add("embeddings", "feat_k", feat_k, r32["k"], r64["k"], rtol=rtol, atol=1e-4)
    # loss, prob and the gradient norm are single numbers, whose fp32-vs-float64 gap is one signed draw that may land on zero: they
    # share one kind, in units of their own float64 value
    for key, got in (("loss", out["loss"]), ("prob", out["prob"]), ("gn", out["grad_norm"])):
        ref = float(r64[key])
        bars.add("loss / prob / gradient norm", key, torch.as_tensor(got).reshape(()).cpu(), r32[key], r64[key], rtol=0.0,
                 atol=rtol + 1e-5 / max(abs(ref), 1e-12), unit=max(abs(ref), 1e-12))
    gn = float(torch.as_tensor(out["grad_norm"]).reshape(()))
    report.update(loss=float(out["loss"]), loss_f64=float(r64["loss"]), prob=float(out["prob"]), grad_norm=gn, grad_norm_f64=r64["gn"],
                  grad_norm_rule32=r32["gn"])
    # ---- every gradient (the flat buffer is clipped in place, as clip_grad_norm_ clips .grad) against the rounded float64 oracle
    coef = min(1.0, tr.clip_norm / (gn + 1e-6)) if tr.clip_norm > 0 else 1.0
    names = {id(p): n for n, p in model.named_parameters()}
    flat = tr.flat_grad.detach().cpu()
    off = 0
    for _, _, p in grad_params(model):
        n = names[id(p)]
        got = flat[off:off + p.numel()].view_as(p).double() / coef
        off += p.numel()
        scale, _ = grad_bar(n, r64["grads"][n])
        bars.add("gradients", f"d {n}", got, r32["grads"][n], r64["grads"][n], rtol=0.0, atol=1e-3, unit=scale)
    assert off == tr.n_live
    # ---- running statistics and the EMA copy; weights within 2.1 lr of the oracle's (a first Adam step moves a weight by ~lr * sign(g))
    after_m, after_e = _state(model), _state(ema)
    for k, v in after_m.items():
        ref = r64["m"][k]
        if not v.dtype.is_floating_point:
            assert torch.equal(v, ref), k
        elif "running_" in k:
            bars.add("running statistics", f"model {k}", v, r32["m"][k], ref, rtol=rtol, atol=1e-5)
        else:
            torch.testing.assert_close(v.double(), ref, rtol=5e-3, atol=2.1 * lr, msg=lambda m, k=k: f"model {k}: {m}")
    for k, v in after_e.items():
        ref = r64["e"][k]
        if v.dtype.is_floating_point:
            bars.add("model_ema", f"model_ema {k}", v, r32["e"][k], ref, rtol=rtol, atol=2e-5)
        else:
            assert torch.equal(v, ref), k
    bars.check()
    report["bars"] = bars
    # ---- queue: rows [index0, index0 + B) are exactly the step's own keys, every other row untouched (memory_moco.py:55-61)
    mem = contrast.memory.detach().cpu()
    ids = (torch.arange(B) + index0) % K
    assert torch.equal(mem[ids], feat_k)
    rest = torch.ones(K, dtype=torch.bool)
    rest[ids] = False
    assert torch.equal(mem[rest], mem0[rest])
    assert int(contrast.index) == (index0 + B) % K
    return report
