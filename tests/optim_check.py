"""The step tails of csrc/step_tail.hip -- Adam's (gcc_adam_step, gcc_adam_ema_step[_scalars], gcc_adam_ema_enqueue_step_scalars,
gcc_adam_clipvalue_step) and SGD's / Adagrad's (gcc_opt_step, gcc_opt_ema_step[_scalars], gcc_opt_clipvalue_step): ONE kernel per
clip kind, so one checker over all three rules -- through the C ABI, shared by tests/test_optim_emu.py (the wave64 emulator
build, CPU tensors) and tests/test_optim_gpu.py (the gfx950 library on cuda:0): only the library, the pointer function and the
device differ.

Reference: torch.optim.SGD / torch.optim.Adagrad on CPU float32, torch.optim.Adam on CPU float64 (its hyper-parameters at the
float values the C ABI receives), behind torch.nn.utils.clip_grad_norm_ (clip_grad_value_ for the fine-tuning tail), four
consecutive steps on fresh gradients whose scale alternates 3.0 / 0.01 (the clip bites on some steps and idles on others) and
whose every 7th element is exactly 0.  Everything a call leaves behind is compared after every step -- parameters, the rule's
state, the clipped gradient stored back, the norm, the EMA copy, the meters -- at tests/nce_check.py's ADAM tolerance (rtol 1e-5,
atol 1e-7): a float32 / fma restatement of the two rules sits within 0.16 (SGD) and 0.025 (Adagrad) of that bound against torch
over four steps, so the reference leaves a factor of six and a wrong operation order (weight decay in front of the clip, eps
inside the sqrt) does not fit.

Sizes: tests/nce_check.py's ADAM_N around the 256-thread workgroup and the sum of squares' 8-load round, and CAP_N around the
update launch's cap of 512 workgroups (131,072 elements), above which a thread takes a second trip of the grid-stride loop and
the element it prefetched next to the norm is no longer its only one; with an EMA tail of 37, n = 131,071 crosses the cap by
n_ema alone."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gcc_amd import _cabi
from tests.nce_check import ADAM, ADAM_N, ADAM_TAILS, _f32, bits, close, cpu, head  # noqa: F401  (head: the tiers' fixture)

SGD, ADAGRAD = 1, 2
RULES = {"sgd": SGD, "adagrad": ADAGRAD}              # (Adam: entry points of its own, no rule number)
ALL_RULES = ["adam", "sgd", "adagrad"]
LR, EPS, EMA_M, STEPS = 0.005, 1e-10, 0.999, 4
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
SCALES = (3.0, 0.01, 3.0, 0.01)
VARIATIONS = (("adam", (BETAS,)), ("sgd", (0.0, 0.9)), ("adagrad", (0.0, 0.01)))       # betas / momentum / lr_decay
# (rule, its variation, weight decay, max_norm, grad_scale) at a size with a ragged last workgroup
NORM_GRID = [(r, v, wd, mn, gs) for r, vs in VARIATIONS for v in vs for wd in (0.0, 1e-5) for mn in (1.0, 0.0, -1.0) for gs in (1.0, 0.5)]
VALUE_GRID = [(r, v, wd, cv, gs) for r, vs in VARIATIONS for v in vs for wd in (0.0, 1e-5) for cv in (1.0, 0.0) for gs in (1.0, 0.5)]
GRID_N = 257
CAP_N = [131071, 131072, 131073]
FOLD_NPARTS = [1, 255, 1024, 1025, 4096]


def gradient(n, scale, gen):
    """a fresh gradient of norm about ``scale`` whose every 7th element is exactly 0"""
    g = torch.randn(n, generator=gen) * (scale / max(n, 1) ** 0.5)
    g[::7] = 0.0
    return g


def rate(rule, t, lr_decay):
    """the rate of step ``t`` as the flat optimizers hand it over: Adagrad's clr in double, as torch forms it"""
    return LR / (1 + (t - 1) * lr_decay) if rule == "adagrad" else LR


def defaults(rule, var):
    """-> (the rule's variation, what the kernel takes as ``hyper``, the number of state tensors)"""
    var = dict(adam=BETAS, sgd=0.9, adagrad=0.01)[rule] if var is None else var
    return var, dict(adam=ADAM_EPS, sgd=var, adagrad=EPS)[rule], 2 if rule == "adam" else 1


def ref_dtype(rule):
    return torch.float64 if rule == "adam" else torch.float32


def torch_optimizer(rule, p, var, wd):
    if rule == "adam":
        return torch.optim.Adam([p], lr=_f32(LR), betas=(_f32(var[0]), _f32(var[1])), eps=_f32(ADAM_EPS), weight_decay=_f32(wd),
                                foreach=False)
    if rule == "sgd":
        return torch.optim.SGD([p], lr=LR, momentum=var, weight_decay=wd, foreach=False)
    return torch.optim.Adagrad([p], lr=LR, lr_decay=var, weight_decay=wd, eps=EPS, foreach=False)


def torch_states(rule, opt, p, var, wd, p_before):
    """what the kernel's state tensors hold: Adam's exp_avg / exp_avg_sq, SGD's momentum buffer (with momentum 0 torch keeps
    none: the kernel's buffer is the step's g' = g_clipped + wd p) or Adagrad's sum"""
    if rule == "adam":
        return [opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]]
    if rule == "adagrad":
        return [opt.state[p]["sum"]]
    if var == 0.0:
        return [p.grad + wd * p_before]
    return [opt.state[p]["momentum_buffer"]]


def fake_views(S, B=5):
    """two batches as far as the meters read them: node_off / edge_off int32[B + 1]"""
    gen = torch.Generator().manual_seed(B)
    def view():
        no = torch.cat([torch.zeros(1, dtype=torch.int64), torch.randint(3, 40, (B,), generator=gen).cumsum(0)]).int()
        eo = torch.cat([torch.zeros(1, dtype=torch.int64), torch.randint(3, 90, (B,), generator=gen).cumsum(0)]).int()
        return SimpleNamespace(node_off=S.t(no), edge_off=S.t(eo), batch_size=B)
    return view(), view()


def run_norm(S, rule, n, tail=None, var=None, wd=1e-5, max_norm=1.0, grad_scale=1.0, mode="value", meters=False, compare=True,
             zero_grad=False):
    """Four steps of the clip-by-norm tail; -> dict of what they left on the device.  ``tail`` None: gcc_adam_step / gcc_opt_step;
    else gcc_adam_ema_step / gcc_opt_ema_step with n_ema = n + tail.  ``mode``: "value", "scalars" (the rate -- and Adam's bias
    corrections -- from a device gcc_step_scalars) or "ema_null" (the _ema_step entry point with ema = meters = NULL).
    ``compare``: against torch after every step."""
    var, hyper, nstate = defaults(rule, var)
    n_all = n + (tail or 0)
    case = f"{rule} n {n} tail {tail} var {var} wd {wd} max_norm {max_norm} scale {grad_scale} {mode}"
    gen = torch.Generator().manual_seed(97 * n + (tail or 0))
    flat0, ema0 = torch.randn(n_all, generator=gen), torch.randn(n_all, generator=gen)
    eng, st = S.engine(), S.stream()
    flat, ema = S.t(flat0), S.t(ema0) if tail is not None else None
    param = flat[:n]
    grad, states = S.t(torch.zeros(n)), [S.t(torch.zeros(n)) for _ in range(nstate)]
    gn, scratch = S.t(torch.zeros(1)), S.t(torch.zeros(64, dtype=torch.float64))
    scalars = S.t(torch.zeros(24, dtype=torch.uint8)) if mode == "scalars" else None
    mt, racc, rmx = None, torch.zeros(5, dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
    if meters:
        q, k = fake_views(S)
        loss, prob = S.t(torch.tensor([1.75])), S.t(torch.tensor([0.125]))
        acc, mx = S.t(torch.zeros(5, dtype=torch.float64)), S.t(torch.zeros(2, dtype=torch.int32))
        mt = (acc, mx, loss, prob, q, k)
    rp = torch.nn.Parameter(flat0[:n].to(ref_dtype(rule)))
    rfull, re = flat0.to(ref_dtype(rule)), ema0.double()
    m64 = float(torch.tensor(EMA_M, dtype=torch.float32))                          # the momentum as the C ABI receives it
    opt = torch_optimizer(rule, rp, var, wd)
    for t in range(1, STEPS + 1):
        g = torch.zeros(n) if zero_grad else gradient(n, SCALES[t - 1], gen)
        grad.copy_(S.t(g))
        lr_t = rate(rule, t, var)
        extras = dict(ema=ema, ema_src=flat if ema is not None else None, ema_m=EMA_M, meters=mt, scalars=scalars)
        if scalars is not None:
            eng.set_scalars(scalars, lr_t, var if rule == "adam" else (0.0, 0.0), t, 0, 0, stream=st)
        if mode == "ema_null" and rule == "adam":
            _cabi.call(S.lib, "gcc_adam_ema_step", S.ptr(param), S.ptr(grad), S.ptr(states[0]), S.ptr(states[1]), n, lr_t, *var, hyper,
                       wd, t, max_norm, grad_scale, S.ptr(gn), S.ptr(scratch), None, 0, 0.0, None, st)
        elif mode == "ema_null":
            _cabi.call(S.lib, "gcc_opt_ema_step", RULES[rule], S.ptr(param), S.ptr(grad), S.ptr(states[0]), n, lr_t, hyper, wd, max_norm,
                       grad_scale, S.ptr(gn), S.ptr(scratch), None, 0, 0.0, None, st)
        elif rule != "adam":
            eng.opt_step(RULES[rule], param, grad, states[0], lr_t, hyper, wd, max_norm, gn, scratch, stream=st, grad_scale=grad_scale,
                         **extras)
        elif ema is None and mt is None and scalars is None:
            eng.adam(param, grad, *states, lr_t, var, hyper, wd, t, max_norm, gn, scratch, stream=st, grad_scale=grad_scale)
        else:
            eng.adam_ema(param, grad, *states, lr_t, var, hyper, wd, t, max_norm, gn, scratch, stream=st, grad_scale=grad_scale, **extras)
        assert cpu(scratch).view(torch.int32)[2:4].tolist() == [0, 0]            # the arrival counter is back at 0
        if not compare:
            continue
        rp.grad = g.to(rp.dtype) * grad_scale                                      # (0.5: exact)
        norm = torch.nn.utils.clip_grad_norm_([rp], max_norm) if max_norm > 0 else rp.grad.norm()
        if n >= 255 and max_norm > 0 and grad_scale == 1.0 and not zero_grad:
            assert (float(norm) > max_norm) == (SCALES[t - 1] > 1)                 # the clip bites / idles as planned
        p_before = rp.detach().clone()
        opt.step()
        rfull[:n] = rp.detach()
        re = re * m64 + (1 - m64) * rfull.double()     # moment_update in float64 (as tests/nce_check.py::check_adam: a float32
        #                                                 restatement drifts by its own roundings, two per step)
        close(case, f"step {t} grad norm", gn.reshape(()), norm.reshape(()), **ADAM)
        close(case, f"step {t} clipped gradient", grad, rp.grad, **ADAM)
        close(case, f"step {t} parameters", param, rp.detach(), **ADAM)
        for i, (mine, ref) in enumerate(zip(states, torch_states(rule, opt, rp, var, wd, p_before))):
            close(case, f"step {t} state {i}", mine, ref.detach(), **ADAM)
        if ema is not None:
            close(case, f"step {t} EMA copy", ema.double(), re, **ADAM)
            assert torch.equal(cpu(flat[n:]), flat0[n:])                           # past the live prefix: only averaged
        if meters:
            nq, nk, eq = (int(x) for x in (cpu(q.node_off)[-1], cpu(k.node_off)[-1], cpu(q.edge_off)[-1]))
            racc += torch.tensor([1.75, 0.125, float(norm), nq + nk, 1.0], dtype=torch.float64)
            rmx = torch.maximum(rmx, torch.tensor([nq, eq], dtype=torch.int32))
            close(case, f"step {t} meters", mt[0], racc, rtol=1e-5, atol=1e-7)
            assert torch.equal(cpu(mt[1]), rmx)
    out = dict(param=param, state=states[0], grad=grad, grad_norm=gn, flat=flat)
    if nstate == 2:
        out["state2"] = states[1]
    if ema is not None:
        out["ema"] = ema
    if meters:
        out["acc"], out["mx"] = mt[0], mt[1]
    return out


def run_value(S, rule, n, var=None, wd=1e-5, clip=1.0, grad_scale=1.0, compare=True):
    """four steps of gcc_adam_clipvalue_step / gcc_opt_clipvalue_step against clip_grad_value_ + torch.optim"""
    from gcc_amd.finetune import ClsHeadEngine

    var, hyper, nstate = defaults(rule, var)
    case = f"{rule} clip-by-value n {n} var {var} wd {wd} clip {clip} scale {grad_scale}"
    gen = torch.Generator().manual_seed(89 * n)
    p0 = torch.randn(n, generator=gen)
    eng, st = ClsHeadEngine(lib=S.lib, ptr=S.ptr), S.stream()
    param, grad, states = S.t(p0), S.t(torch.zeros(n)), [S.t(torch.zeros(n)) for _ in range(nstate)]
    rp = torch.nn.Parameter(p0.to(ref_dtype(rule)))
    opt = torch_optimizer(rule, rp, var, wd)
    for t in range(1, STEPS + 1):
        g = gradient(n, 0.5 * SCALES[t - 1] * n ** 0.5, gen)                       # elements of size ~1.5 / ~0.005: both sides of 1.0
        grad.copy_(S.t(g))
        if rule == "adam":
            eng.adam_clipvalue(param, grad, *states, LR, var, hyper, wd, t, clip, grad_scale=grad_scale, stream=st)
        else:
            eng.opt_clipvalue(RULES[rule], param, grad, states[0], rate(rule, t, var), hyper, wd, clip, grad_scale=grad_scale, stream=st)
        if not compare:
            continue
        rp.grad = g.to(rp.dtype) * grad_scale
        if clip > 0:
            torch.nn.utils.clip_grad_value_([rp], clip)
        p_before = rp.detach().clone()
        opt.step()
        close(case, f"step {t} clipped gradient", grad, rp.grad, **ADAM)
        close(case, f"step {t} parameters", param, rp.detach(), **ADAM)
        for i, (mine, ref) in enumerate(zip(states, torch_states(rule, opt, rp, var, wd, p_before))):
            close(case, f"step {t} state {i}", mine, ref.detach(), **ADAM)
    return dict(param=param, grad=grad, **{f"state{i}": x for i, x in enumerate(states)})


def same_bits(a, b, what):
    for key in a:
        assert torch.equal(bits(a[key]) if a[key].dtype == torch.float32 else cpu(a[key]),
                           bits(b[key]) if b[key].dtype == torch.float32 else cpu(b[key])), f"{what}: {key} differs"


# ---------------------------------------------------------------------------------------------------------------- the checks
def check_norm_sizes(S, rule, n, tail):
    """every size around the 256-thread workgroup, the 8-load round and the 512-workgroup cap, without (tail None) and with the EMA
    copy and the meters"""
    run_norm(S, rule, n, tail, meters=tail is not None)


def check_norm_grid(S, rule, var, wd, max_norm, grad_scale):
    run_norm(S, rule, GRID_N, 37, var=var, wd=wd, max_norm=max_norm, grad_scale=grad_scale, meters=True)


def check_value_sizes(S, rule, n):
    run_value(S, rule, n)


def check_value_grid(S, rule, var, wd, clip, grad_scale):
    run_value(S, rule, GRID_N, var=var, wd=wd, clip=clip, grad_scale=grad_scale)


def check_adagrad_zero_gradient(S):
    """an all-zero gradient on zero state (no weight decay): 0 / (0 + eps) is 0, the parameters keep their bits"""
    for n in (1, 257):
        out = run_norm(S, "adagrad", n, wd=0.0, zero_grad=True)
        gen = torch.Generator().manual_seed(97 * n)
        assert torch.isfinite(cpu(out["param"])).all()
        assert torch.equal(cpu(out["param"]), torch.randn(n, generator=gen))
        assert not cpu(out["state"]).any()
    p, g, s = S.t(torch.ones(5)), S.t(torch.zeros(5)), S.t(torch.zeros(5))
    _cabi.call(S.lib, "gcc_opt_clipvalue_step", ADAGRAD, S.ptr(p), S.ptr(g), S.ptr(s), 5, LR, EPS, 0.0, 1.0, 1.0, S.stream())
    assert torch.equal(cpu(p), torch.ones(5))


def check_scalars_give_the_by_value_bits(S, rule):
    """gcc_adam_ema_step_scalars / gcc_opt_ema_step_scalars read the step's rate (Adagrad: a clr that changes every step) and
    Adam's bias corrections from the device struct"""
    a = run_norm(S, rule, 8193, 37, meters=True, compare=False)
    b = run_norm(S, rule, 8193, 37, meters=True, compare=False, mode="scalars")
    same_bits(a, b, f"{rule}: scalars against by-value")


def check_identical_calls_give_identical_bits(S, rule):
    same_bits(run_norm(S, rule, 8193, 37, meters=True, compare=False), run_norm(S, rule, 8193, 37, meters=True, compare=False),
              f"{rule}: two runs")
    same_bits(run_value(S, rule, 8193, compare=False), run_value(S, rule, 8193, compare=False), f"{rule}: two clip-by-value runs")


def check_ema_step_without_extras_is_opt_step(S, rule):
    same_bits(run_norm(S, rule, 8193, compare=False), run_norm(S, rule, 8193, compare=False, mode="ema_null"),
              f"{rule}: the _ema_step entry point with ema = meters = NULL against the plain one")


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def check_folded_partials(S, nparts, n=8193, tail=37):
    """Adam with the sum of squares handed over as ``nparts`` partials (gcc_adam_ema_enqueue_step_scalars: every workgroup adds
    them up, the first four per thread in the prologue's clamped loads, the rest in the loop behind it) against the call with
    the sum-of-squares launch (gcc_adam_ema_step_scalars), two steps, the first clipped and the second not.  The partials are
    the gradient's squares summed by the host in float64 into ``nparts`` contiguous pieces; whatever lies behind them in the
    buffer is NaN.  grad_norm within one ulp; everything else bit for bit while the norms have been equal, at the flat Adam's
    tolerance (rtol 1e-5, atol 1e-7) after that."""
    gen = torch.Generator().manual_seed(7 * nparts + n)
    flat0, ema0 = torch.randn(n + tail, generator=gen), torch.randn(n + tail, generator=gen)
    grads = [gradient(n, scale, gen) for scale in SCALES[:2]]
    eng, st = S.engine(), S.stream()
    sides = []
    for folded in (False, True):
        flat, ema = S.t(flat0), S.t(ema0)
        grad, m, v = (S.t(torch.zeros(n)) for _ in range(3))
        gn, scratch, scalars = S.t(torch.zeros(1)), S.t(torch.zeros(64, dtype=torch.float64)), S.t(torch.zeros(24, dtype=torch.uint8))
        q, k = fake_views(S)
        mt = (S.t(torch.zeros(5, dtype=torch.float64)), S.t(torch.zeros(2, dtype=torch.int32)), S.t(torch.tensor([1.75])),
              S.t(torch.tensor([0.125])), q, k)
        steps = []
        for t, g in enumerate(grads, 1):
            grad.copy_(S.t(g))
            eng.set_scalars(scalars, LR, BETAS, t, 0, 0, stream=st)
            kw = {}
            if folded:
                parts = torch.full((4096 + 8,), float("nan"), dtype=torch.float64)
                parts[:nparts] = torch.stack([x.sum() for x in torch.tensor_split(g.double().pow(2), nparts)])
                kw = dict(sumsq_parts=(S.t(parts), nparts))
            eng.adam_ema(flat[:n], grad, m, v, 0.0, BETAS, ADAM_EPS, 1e-5, 0, 1.0, gn, scratch, stream=st, ema=ema, ema_src=flat,
                         ema_m=EMA_M, meters=mt, scalars=scalars, **kw)
            steps.append([cpu(x).clone() for x in (gn, flat, ema, m, v, grad, mt[0], mt[1])])
        sides.append(steps)
    exact = True
    for t, (a, b) in enumerate(zip(*sides), 1):
        gn_a, gn_b = float(a[0]), float(b[0])
        print(f"nparts {nparts} step {t}: grad_norm separate {gn_a!r} folded {gn_b!r}")
        assert (gn_a > 1.0) == (t == 1) and _ulps(gn_a, gn_b) <= 1
        exact = exact and gn_a == gn_b
        for x, y in zip(a[1:], b[1:]):
            torch.testing.assert_close(x, y, **(dict(rtol=0, atol=0) if exact else ADAM))


def check_refusals(S):
    """an unknown rule, n = 0 and a NULL state are refused by name, by all four entry points, and touch nothing"""
    p, g, s = S.t(torch.ones(8)), S.t(torch.ones(8)), S.t(torch.ones(8))
    gn, scratch, sc = S.t(torch.zeros(1)), S.t(torch.zeros(64, dtype=torch.float64)), S.t(torch.zeros(24, dtype=torch.uint8))
    st = S.stream()

    def calls(rule, n, state):
        a = (rule, S.ptr(p), S.ptr(g), state, n)
        tail = (1.0, 1.0, S.ptr(gn), S.ptr(scratch))
        yield "gcc_opt_step", a + (LR, 0.9, 0.0) + tail + (st,)
        yield "gcc_opt_ema_step", a + (LR, 0.9, 0.0) + tail + (None, 0, 0.0, None, st)
        yield "gcc_opt_ema_step_scalars", a + (0.9, 0.0) + tail + (None, 0, 0.0, None, S.ptr(sc), st)
        yield "gcc_opt_clipvalue_step", a + (LR, 0.9, 0.0, 1.0, 1.0, st)

    for (rule, n, state), text in (((0, 8, S.ptr(s)), "unknown rule 0"), ((3, 8, S.ptr(s)), "unknown rule 3"),
                                   ((SGD, 0, S.ptr(s)), "n = 0"), ((ADAGRAD, 8, None), "state is NULL")):
        for name, args in calls(rule, n, state):
            with pytest.raises(RuntimeError, match=f"{name} failed.*{name}: {text}"):
                _cabi.call(S.lib, name, *args)
    assert all(torch.equal(cpu(x), torch.ones(8)) for x in (p, g, s))
