"""The fine-tuning head (gcc_amd/csrc/cls_head.hip), clip-by-value Adam (csrc/step_tail.hip) and FinetuneTrainStep on the emulator build, against
float64 torch and against tests/golden/finetune_golden.pt (the reference's own encoder inside its train_finetune)."""
import pytest
import torch
import torch.nn.functional as F

from gcc_amd.finetune import ClsHeadEngine
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_encoder import emu_engine


def emu_head():
    return ClsHeadEngine(lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr())


def _case(B, C, D, seed):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(B, D, generator=g)
    W = torch.randn(C, D, generator=g) * 0.2
    b = torch.randn(C, generator=g) * 0.1
    y = torch.randint(0, C, (B,), generator=g, dtype=torch.int32)
    if B > 2:
        y[-2:] = -1                                             # padding rows
    if B > 1:
        feat[0] = 0.0                                           # row 0: every logit equals its bias ...
        b[:] = 0.0
        b[C - 1] = b[C - 2] = 0.5                               # ... with a tie between the last two classes
    return feat, W, b, y


@pytest.mark.parametrize("B", [1, 7, 32, 65, 256])
@pytest.mark.parametrize("C", [2, 5, 64])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_head_matches_float64_torch(B, C, D):
    feat, W, b, y = _case(B, C, D, B * 1000 + C * 10 + D)
    ld = D + 3                                                  # a row stride wider than D (the padded 64-column buffers)
    fbuf = torch.zeros(B, ld)
    fbuf[:, :D] = feat
    dW, db, dfeat = torch.full((C, D), 7.0), torch.full((C,), 7.0), torch.full((B, ld), 7.0)
    out = emu_head().train(fbuf, W, b, y, dW, db, dfeat)
    valid = y >= 0
    f, Wd, bd = feat.double().requires_grad_(), W.double().requires_grad_(), b.double().requires_grad_()
    logits = f @ Wd.t() + bd
    if valid.any():
        loss = F.cross_entropy(logits[valid], y[valid].long())
        loss.backward()
        torch.testing.assert_close(out["loss"].double().reshape(()), loss.detach(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(dW.double(), Wd.grad, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(db.double(), bd.grad, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(dfeat[:, :D].double(), f.grad, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(out["logits"].double(), logits.detach(), rtol=1e-5, atol=1e-5)
    assert torch.all(dfeat[:, D:] == 0)
    pred = out["logits"].argmax(1)                               # torch.argmax: lowest index among ties
    assert torch.equal(pred, torch.argmax(logits.detach().float(), 1)) or B == 1
    if B > 1:
        assert int(pred[0]) == C - 2                            # the tie of row 0 goes to the lower index
    assert int(out["correct"][0]) == int((pred[valid] == y[valid].long()).sum())
    assert int(out["correct"][1]) == int(valid.sum())


def test_head_refuses_65_classes():
    feat, W, b, y = _case(8, 65, 64, 1)
    with pytest.raises(ValueError):
        emu_head().train(feat, W, b, y, torch.zeros(65, 64), torch.zeros(65), torch.zeros(8, 64))
    # the library itself refuses too (rc < 0 and gcc_last_error), never a truncated result
    import ctypes

    from gcc_amd import _cabi

    lib = emu_lib()
    a = _cabi.GccClsHeadArgs(feat=feat.data_ptr(), W=W.data_ptr(), b=b.data_ptr(), labels=y.data_ptr(), B=8, D=64, C=65,
                             ld_feat=64, ld_dfeat=64)
    assert lib.gcc_cls_head_train(ctypes.byref(a), None) < 0
    assert b"num_classes" in lib.gcc_last_error()


def test_head_eval_accumulates_over_batches():
    eng = emu_head()
    loss_sum, counts = torch.zeros(1, dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
    want_loss, want_correct, want_rows = 0.0, 0, 0
    for B, seed in ((32, 1), (7, 2)):
        feat, W, b, y = _case(B, 5, 64, seed)
        eng.eval(feat, W, b, y, loss_sum, counts)
        v = y >= 0
        logits = feat.double() @ W.double().t() + b.double()
        want_loss += float(F.cross_entropy(logits[v], y[v].long(), reduction="sum"))
        want_correct += int((logits[v].argmax(1) == y[v].long()).sum())
        want_rows += int(v.sum())
    assert abs(float(loss_sum) - want_loss) < 1e-4 * want_rows
    assert counts.tolist() == [want_correct, want_rows]


def test_head_is_bit_identical_run_to_run():
    feat, W, b, y = _case(65, 5, 64, 3)
    res = []
    for _ in range(2):
        dW, db, dfeat = torch.zeros(5, 64), torch.zeros(5), torch.zeros(65, 64)
        out = emu_head().train(feat, W, b, y, dW, db, dfeat)
        res.append((out["loss"].clone(), dW.clone(), db.clone(), dfeat.clone()))
    for a, c in zip(*res):
        assert torch.equal(a, c)


def test_adam_clipvalue_matches_clip_grad_value_and_torch_adam():
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(1000, generator=g)
    ref = p0.clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=0.01, betas=(0.9, 0.999), weight_decay=1e-3)
    p, m, v = p0.clone(), torch.zeros(1000), torch.zeros(1000)
    eng = emu_head()
    for step in range(1, 5):
        grad = torch.randn(1000, generator=g) * 2.0              # many entries beyond the clip value
        ref.grad = grad.clone()
        torch.nn.utils.clip_grad_value_([ref], 1.0)
        opt.step()
        gbuf = grad.clone()
        eng.adam_clipvalue(p, gbuf, m, v, 0.01, (0.9, 0.999), 1e-8, 1e-3, step, 1.0)
        torch.testing.assert_close(gbuf, ref.grad)
        torch.testing.assert_close(p, ref.detach(), rtol=1e-5, atol=1e-6)


def test_finetune_step_reproduces_reference_golden():
    from tests.finetune_check import check_eval, check_steps, run_steps

    model, head, step, outs = run_steps("cpu", gin_engine=emu_engine(), head_engine=emu_head())
    check_steps(model, step, outs)
    check_eval(model, head, "cpu", head_engine=emu_head())
