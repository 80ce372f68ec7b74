"""Shared by tests/test_cls_head_edges_emu.py and tests/test_cls_head_edges_gpu.py: the fine-tuning head and clip-by-value Adam
(csrc/cls_head.hip, csrc/step_tail.hip) at their shape edges against float64 torch (``F.cross_entropy`` on ``feat @ W.T + b``; ``clip_grad_value_`` +
``torch.optim.Adam``).  TEST INFRASTRUCTURE ONLY.

Inputs are generated on the CPU from fixed seeds and then moved (tests/wide_edges_check.py::Tier): both tiers run the same numbers.

Bars: those of tests/test_finetune_emu.py, none chosen here -- loss rtol 1e-5 / atol 1e-6, gradients (dW, db, dfeat, dlogits)
rtol 1e-4 / atol 1e-6, logits rtol 1e-5 / atol 1e-5, the eval sums 1e-4 * rows, Adam rtol 1e-5 / atol 1e-6.

The shapes (B, C, D): C that leaves idle lanes in a wave (R = 64 / C rows per group: C = 1, 3, 21, 33, 63) and C = 64; D that is no
multiple of 4 (the scalar tail of the dot product) down to D = 1; B on both sides of the 1024 threads and of 2048, where the one
workgroup walks the rows; B = 1.  Every shape runs with padding on the tail rows, scattered over ~40 % of the rows, and on every
row.  ``feat`` and ``dfeat`` live in buffers of row stride D + 3 whose extra feat columns hold 1e30."""
import torch
import torch.nn.functional as F

SHAPES = [(1, 1, 1), (3, 1, 5), (22, 3, 3), (21, 3, 4), (65, 3, 65), (64, 33, 7), (130, 63, 255), (127, 64, 255), (1024, 64, 1),
          (1025, 21, 100), (2049, 7, 64)]
PATTERNS = ("tail", "scattered", "all")
LOSS = dict(rtol=1e-5, atol=1e-6)
GRAD = dict(rtol=1e-4, atol=1e-6)
LOGITS = dict(rtol=1e-5, atol=1e-5)
ADAM = dict(rtol=1e-5, atol=1e-6)
PAD = 3


def make_case(B, C, D, pattern, w_scale=1.0):
    """-> (feat [B, D], W [C, D], b [C], labels int32 [B]) on the CPU"""
    g = torch.Generator().manual_seed(B * 100003 + C * 1009 + D * 7 + PATTERNS.index(pattern))
    feat = torch.randn(B, D, generator=g)
    W = torch.randn(C, D, generator=g) * (0.2 * w_scale)
    b = torch.randn(C, generator=g) * 0.1
    y = torch.randint(0, C, (B,), generator=g, dtype=torch.int32)
    if pattern == "tail":
        npad = min(B - 1, max(1, B // 8))
        if npad:
            y[B - npad:] = -1
    elif pattern == "scattered":
        y[torch.rand(B, generator=g) < 0.4] = -1
    else:
        y[:] = -1
    return feat, W, b, y


def reference(feat, W, b, y):
    """float64 torch -> dict(logits, loss, dW, db, dfeat, dlogits, valid): the mean cross entropy over the rows with a label,
    0 and zero gradients without one"""
    f, Wd, bd = feat.double().requires_grad_(), W.double().requires_grad_(), b.double().requires_grad_()
    logits = f @ Wd.t() + bd
    logits.retain_grad()
    valid = y >= 0
    if bool(valid.any()):
        loss = F.cross_entropy(logits[valid], y[valid].long())
        loss.backward()
        return dict(logits=logits.detach(), loss=loss.detach(), dW=Wd.grad, db=bd.grad, dfeat=f.grad, dlogits=logits.grad, valid=valid)
    z = torch.zeros
    return dict(logits=logits.detach(), loss=z((), dtype=torch.float64), dW=z(W.shape, dtype=torch.float64),
                db=z(b.shape, dtype=torch.float64), dfeat=z(feat.shape, dtype=torch.float64),
                dlogits=z(logits.shape, dtype=torch.float64), valid=valid)


def run_train(tier, feat, W, b, y, eng=None):
    """the head's train call on strided buffers -> dict of CPU tensors: loss, correct, logits, dlogits, dW, db, dfeat [B, D + 3]"""
    B, D = feat.shape
    C = W.shape[0]
    fbuf = torch.full((B, D + PAD), 1e30)
    fbuf[:, :D] = feat
    dW, db, dfeat = tier.to(torch.full((C, D), 7.0)), tier.to(torch.full((C,), 7.0)), tier.to(torch.full((B, D + PAD), 7.0))
    out = (eng or tier.head_engine()).train(tier.to(fbuf), tier.to(W), tier.to(b), tier.to(y), dW, db, dfeat)
    tier.sync()
    res = {k: v.cpu() for k, v in out.items()}
    res.update(dW=dW.cpu(), db=db.cpu(), dfeat=dfeat.cpu())
    return res


def _share(got, ref):
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def compare(what, res, ref, D):
    """every output of a train call against float64 at the bars; -> the worst error as a share of the tensor's largest entry"""
    msg = lambda k: (lambda m: f"{what}: {k}: {m}")                     # noqa: E731
    torch.testing.assert_close(res["logits"].double(), ref["logits"], msg=msg("logits"), **LOGITS)
    torch.testing.assert_close(res["loss"].double().reshape(()), ref["loss"], msg=msg("loss"), **LOSS)
    torch.testing.assert_close(res["dW"].double(), ref["dW"], msg=msg("dW"), **GRAD)
    torch.testing.assert_close(res["db"].double(), ref["db"], msg=msg("db"), **GRAD)
    torch.testing.assert_close(res["dfeat"][:, :D].double(), ref["dfeat"], msg=msg("dfeat"), **GRAD)
    torch.testing.assert_close(res["dlogits"].double(), ref["dlogits"], msg=msg("dlogits"), **GRAD)
    assert bool((res["dfeat"][:, D:] == 0).all()), f"{what}: the columns of dfeat past D are not exactly zero"
    for k in ("logits", "loss", "dW", "db", "dfeat", "dlogits"):
        assert not bool(torch.isnan(res[k]).any()), f"{what}: {k} holds a NaN"
    worst = max(_share(res[k] if k != "dfeat" else res[k][:, :D], ref[k]) for k in ("logits", "dW", "db", "dfeat", "dlogits")
                if float(ref[k].abs().max()) > 0)
    if float(ref["loss"]) > 0:
        worst = max(worst, abs(float(res["loss"]) - float(ref["loss"])) / float(ref["loss"]))
    return worst


def expected_correct(res, ref, y):
    """[correct, valid] from the kernel's own logits (torch.argmax: the lowest index among ties); the float64 argmax must agree
    on every row whose two largest float64 logits are further apart than the logits' bar"""
    valid = ref["valid"]
    pred = res["logits"].argmax(1)
    if ref["logits"].shape[1] > 1:
        top = ref["logits"].topk(2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > 1e-4 * (1 + top[:, 0].abs())
        assert torch.equal(pred[clear], ref["logits"].argmax(1)[clear])
    return [int((pred[valid] == y[valid].long()).sum()), int(valid.sum())]


def check_shape(tier, B, C, D, pattern):
    feat, W, b, y = make_case(B, C, D, pattern)
    ref = reference(feat, W, b, y)
    res = run_train(tier, feat, W, b, y)
    what = f"head B {B} C {C} D {D} {pattern}"
    worst = compare(what, res, ref, D)
    assert res["correct"].tolist() == expected_correct(res, ref, y), what
    nvalid = int(ref["valid"].sum())
    if pattern == "all":
        assert nvalid == 0
    elif B > 8:
        assert 0 < nvalid < B, "the pattern left no padding row, or no labelled one"
    if nvalid == 0:                                    # an all-padding batch: exact zeros, no 0 / 0
        assert float(res["loss"]) == 0.0 and res["correct"].tolist() == [0, 0], what
        for k in ("dW", "db", "dfeat", "dlogits"):
            assert bool((res[k] == 0).all()), f"{what}: {k} of an all-padding batch is not exactly zero"
    print(f"{what}: worst error vs float64 {worst:.2e} of the tensor's largest entry ({nvalid} labelled rows)")
    return worst


def check_wide_logits(tier):
    """W scaled by 20: a row's logits spread over more than 88, where exp() without the max subtraction overflows fp32"""
    B, C, D = 65, 5, 64
    feat, W, b, y = make_case(B, C, D, "tail", w_scale=20.0)
    ref = reference(feat, W, b, y)
    spread = float((ref["logits"].max(1).values - ref["logits"].min(1).values).max())
    assert spread > 88.0, f"the widest row spreads over {spread:.1f} only: the case lost its point"
    res = run_train(tier, feat, W, b, y)
    worst = compare("head, wide logits", res, ref, D)
    assert res["correct"].tolist() == expected_correct(res, ref, y)
    print(f"head, wide logits (spread {spread:.0f}): worst error vs float64 {worst:.2e} of the tensor's largest entry")
    return worst


def check_ties(tier):
    """C = 5 (12 rows per group): rows 1 and 17 are zero, so their logits are the biases, of which classes 2 and 4 hold the
    bitwise-equal largest.  The prediction is class 2: labelled 2 the rows count as correct, labelled 4 they do not."""
    B, C, D = 30, 5, 64
    feat, W, b, y = make_case(B, C, D, "tail")
    rows = [1, 17]
    assert all(r % (64 // C) != 0 for r in rows) and bool((y[rows] >= 0).all())      # not a group's first row; labelled
    feat[rows] = 0.0
    b[:] = torch.tensor([0.1, -0.2, 0.5, 0.3, 0.5])
    counts = {}
    for label in (2, 4):
        y[rows] = label
        ref = reference(feat, W, b, y)
        res = run_train(tier, feat, W, b, y)
        compare(f"head, ties labelled {label}", res, ref, D)
        for r in rows:
            assert float(res["logits"][r, 2]) == float(res["logits"][r, 4]) == float(res["logits"][r].max())
        others = [r for r in range(B) if r not in rows and int(y[r]) >= 0]
        base = int((res["logits"][others].argmax(1) == y[others].long()).sum())
        counts[label] = res["correct"].tolist()
        assert counts[label] == [base + (len(rows) if label == 2 else 0), int((y >= 0).sum())], (label, counts[label], base)
    return counts


def check_label_out_of_range(tier):
    """a label >= C: the loss is NaN (as the kernel documents), every dlogits entry stays finite"""
    B, C, D = 22, 3, 7
    feat, W, b, y = make_case(B, C, D, "tail")
    y[4], y[13] = C, C + 60
    res = run_train(tier, feat, W, b, y)
    assert bool(torch.isnan(res["loss"]).all()), "an out-of-range label did not give a NaN loss"
    assert bool(torch.isfinite(res["dlogits"]).all())
    assert res["correct"][1].item() == int((y >= 0).sum())


def check_eval(tier):
    """gcc_cls_head_eval twice into one accumulator pair: logits bitwise the train call's, the sums against float64"""
    eng = tier.head_engine()
    loss_sum = tier.to(torch.zeros(1, dtype=torch.float64))
    counts = tier.to(torch.zeros(2, dtype=torch.int32))
    want_loss, want = 0.0, [0, 0]
    for B, C, D in ((65, 3, 65), (1025, 21, 100)):
        feat, W, b, y = make_case(B, C, D, "scattered")
        ref = reference(feat, W, b, y)
        res = run_train(tier, feat, W, b, y, eng=eng)
        fbuf = torch.full((B, D + PAD), 1e30)
        fbuf[:, :D] = feat
        logits = tier.to(torch.full((B, C), 7.0))
        eng.eval(tier.to(fbuf), tier.to(W), tier.to(b), tier.to(y), loss_sum, counts, logits=logits)
        tier.sync()
        assert torch.equal(logits.cpu(), res["logits"]), "eval and train logits differ in their bits"
        v = ref["valid"]
        want_loss += float(F.cross_entropy(ref["logits"][v], y[v].long(), reduction="sum"))
        c = expected_correct(res, ref, y)
        want = [want[0] + c[0], want[1] + c[1]]
    assert abs(float(loss_sum.cpu()) - want_loss) < 1e-4 * want[1], (float(loss_sum.cpu()), want_loss)
    assert counts.cpu().tolist() == want
    return float(loss_sum.cpu()), want_loss


def check_autograd(tier):
    """cls_head_loss through autograd: (3 * loss).backward() leaves three times the float64 gradients (D = 65)"""
    from gcc_amd.finetune import cls_head_loss

    B, C, D = 65, 3, 65
    feat, W, b, y = make_case(B, C, D, "scattered")
    ref = reference(feat, W, b, y)
    head = torch.nn.Linear(D, C)
    with torch.no_grad():
        head.weight.copy_(W)
        head.bias.copy_(b)
    head = tier.to(head)
    f = tier.to(feat).clone().requires_grad_()
    loss, logits, correct = cls_head_loss(f, head, tier.to(y), engine=tier.head_engine())
    (3 * loss).backward()
    tier.sync()
    torch.testing.assert_close(loss.detach().cpu().double(), ref["loss"], **LOSS)
    torch.testing.assert_close(logits.cpu().double(), ref["logits"], **LOGITS)
    torch.testing.assert_close(f.grad.cpu().double(), 3 * ref["dfeat"], **GRAD)
    torch.testing.assert_close(head.weight.grad.cpu().double(), 3 * ref["dW"], **GRAD)
    torch.testing.assert_close(head.bias.grad.cpu().double(), 3 * ref["db"], **GRAD)
    assert correct.cpu().tolist()[1] == int(ref["valid"].sum())


def check_repeatable(tier):
    """two runs of (1025, 21, 100) are bit-identical: no float atomics anywhere"""
    feat, W, b, y = make_case(1025, 21, 100, "scattered")
    a, c = run_train(tier, feat, W, b, y), run_train(tier, feat, W, b, y)
    for k in a:
        assert torch.equal(a[k], c[k]), f"{k} differs between two runs"


def check_adam_clipvalue(tier, n):
    """gcc_adam_clipvalue_step over n elements (its grid stops at 512 x 256 threads: above 131,072 a thread makes a second trip),
    four steps, grad_scale in {1, 0.5}, clip_value in {1, 0}: the parameters, both moments and the stored-back clipped gradient
    against clip_grad_value_ + torch.optim.Adam; torch's fp32 step itself against a float64 restatement of the rule"""
    lr, (b1, b2), eps, wd = 0.01, (0.9, 0.999), 1e-8, 1e-3
    eng = tier.head_engine()
    worst = 0.0
    for grad_scale in (1.0, 0.5):
        for clip in (1.0, 0.0):
            g = torch.Generator().manual_seed(n * 10 + int(grad_scale * 2) + int(clip))
            p0 = torch.randn(n, generator=g)
            ref = p0.clone().requires_grad_()
            opt = torch.optim.Adam([ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
            p, m, v = tier.to(p0.clone()), tier.to(torch.zeros(n)), tier.to(torch.zeros(n))
            p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
            above = below = False
            for step in range(1, 5):
                grad = torch.randn(n, generator=g) * 3.0
                grad[0] = (3.0, 0.2, -3.0, -0.1)[step - 1] / grad_scale
                above |= bool((grad.abs() * grad_scale > 1.0).any())
                below |= bool((grad.abs() * grad_scale < 1.0).any())
                ref.grad = grad * grad_scale
                if clip > 0:
                    torch.nn.utils.clip_grad_value_([ref], clip)
                opt.step()
                g64 = grad.double() * grad_scale
                if clip > 0:
                    g64 = g64.clamp(-clip, clip)
                gi = g64 + wd * p64
                m64 = b1 * m64 + (1 - b1) * gi
                v64 = b2 * v64 + (1 - b2) * gi * gi
                p64 = p64 - lr / (1 - b1 ** step) * m64 / (v64.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
                torch.testing.assert_close(ref.detach().double(), p64, msg=lambda s: f"BAD INPUT, not a kernel error -- torch's fp32 "
                                           f"Adam step is outside the bar against float64: {s}", **ADAM)
                gbuf = tier.to(grad.clone())
                eng.adam_clipvalue(p, gbuf, m, v, lr, (b1, b2), eps, wd, step, clip, grad_scale=grad_scale)
                tier.sync()
                what = f"n {n} grad_scale {grad_scale} clip {clip} step {step}"
                torch.testing.assert_close(gbuf.cpu(), ref.grad, msg=lambda s: f"{what}: stored-back gradient: {s}")
                torch.testing.assert_close(p.cpu(), ref.detach(), msg=lambda s: f"{what}: param: {s}", **ADAM)
                st = opt.state[ref]
                torch.testing.assert_close(m.cpu(), st["exp_avg"], msg=lambda s: f"{what}: exp_avg: {s}", **ADAM)
                torch.testing.assert_close(v.cpu(), st["exp_avg_sq"], msg=lambda s: f"{what}: exp_avg_sq: {s}", **ADAM)
                worst = max(worst, float((p.cpu().double() - p64).abs().max()))
            assert above and below, "the gradients do not span both sides of the clip value"
    print(f"adam_clipvalue n {n}: worst parameter error vs float64 {worst:.2e} absolute")
    return worst
