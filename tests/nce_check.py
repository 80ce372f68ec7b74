"""The MoCo / InfoNCE head (gcc_amd/csrc/nce.hip), the queue enqueue, the EMA update, the gradient norm and Adam
(gcc_amd/csrc/step_tail.hip) against the
reference-generated golden vectors, the oracle and float64 restatements in torch, shared by the emulator tier
(tests/test_nce_emu.py, tests/test_nce_onepass_emu.py) and the GPU tier (tests/test_nce_gpu.py): the same cases and checks; only
the library, the pointer function and the device differ.

References are computed in float64 on the CPU from CPU copies of the inputs; results are copied back for comparison.  Before
every call of the head, check_case and its siblings fill the engine's workspace with 0xFF bytes (NaN partials and slabs, the
ticket at -1): the kernels claim to write everything they later read and to zero the ticket themselves, so a read of an
unwritten partial shows as NaN on either tier.  After every call that counts arrivals the ticket must be back at 0.

Tolerances (the head's own, set on the emulator): loss / prob / lse / pos rtol 1e-5, atol 1e-6; dense logits rtol 1e-5,
atol 1e-5 (bf16: 2e-5); d loss / d q rtol 1e-4, atol 1e-7; Adam rtol 1e-5, atol 1e-7.  Every comparison prints its largest
error next to the bound it was held to (``nce-fig`` lines; profiles/nce_edges_device.txt collects them)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from gcc_amd import _cabi
from gcc_amd.contrast import MemoryMoCo, NceEngine, NCESoftmaxLoss, NCESoftmaxLossNS, e2e_logits
from oracle import encoder as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = torch.load(os.path.join(os.path.dirname(__file__), "golden", "encoder_golden.pt"), weights_only=False)
T = 0.07
SCALAR = dict(rtol=1e-5, atol=1e-6)          # loss / prob / lse / pos
DENSE = dict(rtol=1e-5, atol=1e-5)
DQ = dict(rtol=1e-4, atol=1e-7)
ADAM = dict(rtol=1e-5, atol=1e-7)            # tests/test_train_step_gpu.py::test_gcc_adam_step_matches_torch_adam_with_clipping
OUTS = ("loss", "prob", "lse", "pos")

RAGGED = [(1, 1), (5, 7), (70, 200), (130, 64)]
ONEPASS_B, ONEPASS_K = [1, 63, 64, 65, 256], [64, 100, 200, 4097]
E2E_B = [1, 2, 15, 17, 63, 64, 65, 70, 129, 130, 256]
BIT_SHAPES = [(70, 200), (256, 4097)]
ADAM_N = [1, 63, 255, 256, 257, 8191, 8193]
ADAM_TAILS = [0, 37]


class _Recorder:
    """a library with the names of the C-ABI calls made through it"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._lib, name)


def emu_ptr(t):
    return 0 if t is None else t.data_ptr()


class Head:
    """the library under test, its pointer function and its device (the emulator works on CPU tensors)"""

    def __init__(self, lib, ptr, device):
        self.lib, self.ptr, self.device = lib, ptr, torch.device(device)

    def engine(self, dtype="f32", record=False):
        return NceEngine(lib=_Recorder(self.lib) if record else self.lib, ptr=self.ptr, dtype=dtype)

    def t(self, x):
        """a copy of ``x`` on the device (a copy on the CPU as well: the kernels write in place)"""
        return None if x is None else x.detach().clone().contiguous().to(self.device)

    def stream(self):
        return _cabi.raw_stream(self.device)

    def moco(self, K, T, memory, index=0, dtype="f32"):
        contrast = MemoryMoCo(64, None, K, T, use_softmax=True, nce_dtype=dtype)
        contrast._engine = self.engine(dtype)
        contrast.load_state_dict({"params": torch.tensor([-1]), "memory": memory.clone()})
        contrast.index = index
        return contrast.to(self.device)


def head(tier):
    """``"emu"``: the wave64 emulator build on CPU tensors; ``"gpu"``: the gfx950 library on cuda:0"""
    if tier == "emu":
        from tests.hipemu.emu_driver import emu_lib

        return Head(emu_lib(), emu_ptr, "cpu")
    return Head(_cabi.load(), _cabi.dev_ptr, "cuda:0")


def cpu(x):
    return x.detach().cpu()


def bits(x):
    return cpu(x).contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------- comparisons with their figures
FIGURES = []


def note(case, what, err, bound):
    FIGURES.append((case, what, float(err), float(bound)))
    print(f"nce-fig | {case} | {what} | largest error {float(err):.3e} | bound {float(bound):.3e}")


def close(case, what, got, ref, rtol, atol):
    """torch.testing.assert_close(got, ref) on CPU copies; records the error of the element closest to (or furthest past) its
    bound atol + rtol |ref|"""
    g, r = cpu(got), cpu(ref)
    if g.dtype != r.dtype:
        g = g.to(r.dtype)
    g = g.reshape(r.shape) if g.numel() == r.numel() == 1 else g
    err, allowed = (g.double() - r.double()).abs(), atol + rtol * r.double().abs()
    if err.numel() and torch.isfinite(err).all():
        i = int((err / allowed).argmax())
        note(case, what, err.reshape(-1)[i], allowed.reshape(-1)[i])
    else:
        note(case, what, float("nan"), float(allowed.min()) if allowed.numel() else atol)
    torch.testing.assert_close(g, r, rtol=rtol, atol=atol, msg=lambda m: f"{case}: {what}: {m}")


def within(case, what, got, ref, bound):
    """|got - ref| <= bound everywhere (a bound derived from the formats; see the caller's docstring)"""
    err = (cpu(got).double() - cpu(ref).double()).abs().max()
    note(case, what, err, bound)
    assert err <= bound, f"{case}: {what}: largest error {float(err):.3e} above the bound {bound:.3e}"


# ------------------------------------------------------------------------------------------------------------ the workspace
def poison(eng, B, K, device):
    """0xFF into the workspace the next call at this shape will get: NaN partials and slabs, the ticket at -1"""
    ws, nbytes = eng._workspace(B, K, device)
    ws.fill_(0xFF)
    return ws, nbytes


def ticket(ws, nbytes):
    """the arrival counter: the last 256-byte slot of the plan (make_plan in nce.hip)"""
    return int(ws[nbytes - 256: nbytes - 252].cpu().clone().view(torch.int32)[0])


# ------------------------------------------------------------------------------------------------- inputs and references
def unit_inputs(B, K, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=1)
    k = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=1)
    mem = torch.nn.functional.normalize(torch.randn(K, 64, generator=g), dim=1)
    return q, k, mem


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _patched(mem, patch, patch_index):
    if patch is None:
        return mem
    m = mem.clone()
    K = m.shape[0]
    for i in range(patch.shape[0]):
        m[(patch_index + i) % K] = patch[i]
    return m


def reference_f64(q, k, mem, dloss, patch=None, patch_index=0, T=T):
    q, k, mem = q.double(), k.double(), _patched(mem, patch, patch_index).double()
    B = q.shape[0]
    logits = torch.cat([(q * k).sum(1, keepdim=True), q @ mem.t()], dim=1) / T
    lse = torch.logsumexp(logits, dim=1)
    p = torch.softmax(logits, dim=1)
    dq = float(dloss) / (B * T) * (p[:, 1:] @ mem + (p[:, :1] - 1.0) * k)
    return dict(lse=lse, pos=logits[:, 0], loss=(lse - logits[:, 0]).mean(), prob=logits[:, 0].mean(), dq=dq)


# ----------------------------------------------------------------------------- one-pass == float64 == four launches (MoCo)
def check_case(S, q, k, mem, dloss=1.0, patch=None, patch_index=0, T=T, dq_bound=None, case=None):
    """one-pass == float64 reference == four launches, each at the head's tolerances (``dq_bound``: see
    check_logits_reach_plus_minus_60); every call starts from a workspace of 0xFF bytes and leaves the ticket at 0"""
    B, K = q.shape[0], mem.shape[0]
    case = case or f"moco B {B} K {K} dloss {dloss:g}"
    eng, st = S.engine(), S.stream()
    qd, kd, md, pd = S.t(q), S.t(k), S.t(mem), S.t(patch)
    dl = S.t(torch.tensor([dloss], dtype=torch.float32))
    ws, nbytes = poison(eng, B, K, S.device)
    outs, dq = eng.forward_backward(qd, kd, md, T, dl, patch=pd, patch_index=patch_index, stream=st)
    assert ticket(ws, nbytes) == 0
    poison(eng, B, K, S.device)
    old = eng.forward(qd, kd, md, T, 0, patch=pd, patch_index=patch_index, stream=st)
    assert ticket(ws, nbytes) == 0
    poison(eng, B, K, S.device)
    dq_old = eng.backward(qd, kd, md, T, 0, old, dl, patch=pd, patch_index=patch_index, stream=st)
    ref = reference_f64(q, k, mem, dloss, patch, patch_index, T)
    for name in OUTS:
        close(case, name, outs[name].double(), ref[name], **SCALAR)
        close(case, f"{name} vs four launches", outs[name], old[name], **SCALAR)
        close(case, f"{name} of the four launches", old[name].double(), ref[name], **SCALAR)
    assert torch.isfinite(cpu(dq)).all() and torch.isfinite(cpu(dq_old)).all()
    if dq_bound is not None:
        within(case, "dq", dq, ref["dq"], dq_bound)
        within(case, "dq of the four launches", dq_old, ref["dq"], dq_bound)
        return outs, cpu(dq)
    close(case, "dq", dq.double(), ref["dq"], **DQ)
    close(case, "dq of the four launches", dq_old.double(), ref["dq"], **DQ)
    return outs, cpu(dq)


def check_onepass_shape(S, B, K):
    check_case(S, *unit_inputs(B, K, 1000 * B + K))


def check_more_than_64_slices(tier):
    """GCC_NCE_WGS = 512 (read once per process: a process of its own): K = 8197, B = 8 -> 129 slices of 64 rows, the last of 5;
    the merge kernel's loop over slice blocks runs three times"""
    code = ("import torch\n"
            "from tests import nce_check as C\n"
            f"S = C.head({tier!r})\n"
            "assert S.lib.gcc_nce_workspace_bytes(8, 8197) > 129 * 8 * 64 * 4\n"      # (129 slabs: the plan did take the setting)
            "C.check_case(S, *C.unit_inputs(8, 8197, 5), dloss=0.5)\n")
    env = dict(os.environ, GCC_NCE_WGS="512", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


def _quantised(B, K, seed, scale):
    """operands on a dyadic grid (q, k: 1 / 16; queue: 1 / 8) and T = 1 / 16: every logit is EXACT in fp32"""
    q, k, _ = unit_inputs(B, K, seed)
    g = torch.Generator().manual_seed(seed + 1)
    mem = torch.round(torch.randn(K, 64, generator=g) * scale * 8) / 8
    return torch.round(q * 16) / 16, torch.round(k * 16) / 16, mem


def check_logits_reach_plus_minus_60(S, B, K):
    """Queue rows scaled, not normalised: |logit| reaches 60 and beyond.  A missing rescale, or a fixed reference maximum such
    as 1 / T, overflows or flushes every term to zero here.

    fp32 cannot hold the unit-vector tolerance for dq on arbitrary inputs of this size: lse is an fp32 OUTPUT, at |lse| ~ 70
    its half ulp is 3.8e-6 and every p = exp(l - lse) inherits that as a relative error, as it does the rounding of its own
    logit.  (a) Inputs whose logits are exact in fp32 and whose softmax has one row above all others by more than 2^-24
    relative (lse = the maximum, exactly): rtol 1e-4 / atol 1e-7 as everywhere.  (b) Random scaled rows: loss / prob / lse / pos
    at their tolerances, and dq within what the formats allow -- |dp / p| <= 2^-24 (|lse| + 8 |l|) (8 = sqrt(64) roundings of the
    dot product) <= 9 * 2^-24 max |logit|, times the largest term dloss / (B T) max |queue entry|."""
    T16 = 1.0 / 16
    q, k, mem = _quantised(B, K, 7 * B + K, 1.0)
    pos_rows = 40 + (K // B) * torch.arange(B) if B < 16 else torch.arange(B) * (K // B) + 7
    mem[pos_rows] = 6.0 * q                                       # one row far above the rest per query ...
    mem[(pos_rows + 3) % K] = -6.0 * q                            # ... and one far below
    logits = q @ mem.t() / T16
    top2 = logits.topk(2, dim=1).values
    assert logits.max() > 60 and logits.min() < -60 and ((top2[:, 0] - top2[:, 1]) > 20).all()
    check_case(S, q, k, mem, T=T16, case=f"exact logits to +-60 B {B} K {K}")
    check_case(S, q, k, mem, T=T16, dloss=0.25, case=f"exact logits to +-60 B {B} K {K} dloss 0.25")
    q, k, _ = unit_inputs(B, K, 7 * B + K)                        # (b)
    mem = torch.randn(K, 64, generator=torch.Generator().manual_seed(K)) * 1.5
    logits = torch.cat([q @ mem.t(), 3.0 * (q * k).sum(1, keepdim=True)], 1) / T
    assert logits.max() > 60 and logits.min() < -60
    bound = 9 * 2.0 ** -24 * float(logits.abs().max()) / (B * T) * float(mem.abs().max())
    check_case(S, q, 3.0 * k, mem, dq_bound=bound, case=f"random logits to +-60 B {B} K {K}")      # (a positive logit far above 1 / T as well)


def check_monotonic_maximum(S, order):
    """every query's logit strictly increases along the queue (every tile raises the running maximum: the accumulators are
    rescaled every time) or strictly decreases (never after the first tile)"""
    B, K = 20, 300
    g = torch.Generator().manual_seed(3)
    u = torch.nn.functional.normalize(torch.randn(64, generator=g), dim=0)
    q = torch.nn.functional.normalize(u + 0.05 * torch.randn(B, 64, generator=g), dim=1)
    k = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=1)
    scale = torch.arange(1, K + 1, dtype=torch.float32) * 0.01
    if order == "decreasing":
        scale = scale.flip(0)
    mem = scale[:, None] * u[None, :]
    logits = q @ mem.t() / T
    d = logits[:, 1:] - logits[:, :-1]
    assert (d > 0).all() if order == "increasing" else (d < 0).all()
    check_case(S, q, k, mem, case=f"maximum {order} along the queue")


def check_lane_groups(S):
    """rows 4 g .. 4 g + 3 of every 16-row tile belong to lane group g: with the large logits in ONE lane group's rows only, a
    maximum kept per lane group would weigh the other groups' rows by their own (much smaller) maxima"""
    B, K = 17, 128
    q, k, mem = unit_inputs(B, K, 11)
    big = (torch.arange(K) % 16) // 4 == 2
    mem = torch.where(big[:, None], mem, 0.05 * mem)        # (unit rows at most: the regime the tolerances were set in)
    check_case(S, q, k, mem, case="large logits in one lane group")


def check_patch_rows_and_dloss(S):
    B, K = 70, 200
    q, k, mem = unit_inputs(B, K, 13)
    g = torch.Generator().manual_seed(17)
    patch = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=1)
    outs, dq = check_case(S, q, k, mem, dloss=-2.5, patch=patch, patch_index=170, case="patch wraps at 170, dloss -2.5")   # rows 170..199, 0..39
    _, dq1 = check_case(S, q, k, mem, dloss=1.0, patch=patch, patch_index=170, case="patch wraps at 170")
    torch.testing.assert_close(dq, -2.5 * dq1, rtol=1e-6, atol=0)
    _, dq0 = check_case(S, q, k, mem)
    assert not torch.equal(dq1, dq0)                                               # (the patch is really read)


def check_bf16_keeps_the_four_launches(S):
    """the one-pass kernels are f32; --nce-dtype bf16 stays on gcc_nce_forward + gcc_nce_backward, and the library refuses it"""
    B, K = 6, 48
    q, k, mem = (S.t(x) for x in unit_inputs(B, K, 19))
    st = S.stream()
    eng = S.engine("bf16", record=True)
    assert not eng.one_pass()
    dl = S.t(torch.ones(1))
    outs, dq = eng.forward_backward(q, k, mem, T, dl, stream=st)
    assert "gcc_nce_forward_backward" not in eng.lib.calls and {"gcc_nce_forward", "gcc_nce_backward"} <= set(eng.lib.calls)
    old = eng.forward(q, k, mem, T, 0, stream=st)
    assert torch.equal(cpu(dq), cpu(eng.backward(q, k, mem, T, 0, old, dl, stream=st))) and torch.equal(cpu(outs["loss"]), cpu(old["loss"]))
    f32 = S.engine(record=True)
    f32.forward_backward(q, k, mem, T, dl, stream=st)
    assert "gcc_nce_forward_backward" in f32.lib.calls and "gcc_nce_backward" not in f32.lib.calls
    a = eng._args(q, k, mem, 1.0 / T, 0, None, 0, outs, None)
    assert a.dtype == 1
    ws, nbytes = eng._workspace(B, K, q.device)
    before = bits(dq).clone()
    rc = S.lib.gcc_nce_forward_backward(ctypes.byref(a), S.ptr(dl), S.ptr(dq), S.ptr(ws), nbytes, None, None, st)
    assert rc == -2
    assert torch.equal(bits(dq), before)                                           # (refused before any launch)


# --------------------------------------------------------------------------------- the module-level API against the golden
def check_moco_golden(S):
    g = GOLD["moco"]
    contrast = S.moco(g["K"], g["T"], g["init"]["memory"])
    q, k = S.t(g["feat_q"]).requires_grad_(True), S.t(g["feat_k"])
    case = "MoCo golden B 6 K 48"
    dense_before = contrast.logits(q, k)
    close(case, "dense logits before the enqueue", dense_before, g["out"], **DENSE)
    out = contrast(q, k)
    assert tuple(out.shape) == tuple(g["out"].shape)
    loss = NCESoftmaxLoss()(out)
    close(case, "loss", loss, g["loss"], **SCALAR)
    close(case, "prob from out[:, 0]", out[:, 0].mean(), g["prob"], **SCALAR)
    close(case, "prob", out.prob, g["prob"], **SCALAR)
    # the queue now holds the keys (memory_moco.py:55-61) and the ring pointer advanced
    torch.testing.assert_close(cpu(contrast.memory), g["after"]["memory"])
    assert contrast.index == g["after"]["index"]
    # dense logits on demand are those of the queue BEFORE the enqueue
    close(case, "dense logits", out.dense(), g["out"], **DENSE)
    loss.backward()
    close(case, "dq", q.grad, g["dfeat_q"], **DQ)


def check_ragged_vs_oracle(S, B, K):
    """MemoryMoCo.forward at ragged (B, K) against the oracle.  B > K: the reference's index_copy_ and gcc_queue_enqueue both need
    B <= K, so the head alone is compared there (loss, dense logits, dq through the engine) and the enqueue must refuse."""
    torch.manual_seed(B * 1000 + K)
    q = torch.nn.functional.normalize(torch.randn(B, 64), dim=1)
    k = torch.nn.functional.normalize(torch.randn(B, 64), dim=1)
    mem = E.memory_init(K, 64)
    index0 = K // 3
    case = f"MoCo vs oracle B {B} K {K}"
    qo = q.clone().requires_grad_(True)
    contrast = S.moco(K, 0.07, mem, index0)
    qd, kd = S.t(q).requires_grad_(True), S.t(k)
    if B > K:
        out_ref = torch.cat(((qo * k).sum(dim=1, keepdim=True), qo @ mem.t()), dim=1) / 0.07       # memory_moco.py:40-44, no enqueue
        loss_ref = E.nce_softmax_loss(out_ref)
        loss_ref.backward()
        eng, st = S.engine(), S.stream()
        md = S.t(mem)
        outs = eng.forward(qd.detach(), kd, md, 0.07, 0, dense=True, stream=st)
        dq = eng.backward(qd.detach(), kd, md, 0.07, 0, outs, S.t(torch.ones(1)), stream=st)
        close(case, "loss", outs["loss"], loss_ref.detach(), **SCALAR)
        close(case, "dense logits", outs["out"], out_ref.detach(), **DENSE)
        close(case, "dq", dq, qo.grad, **DQ)
        with pytest.raises(RuntimeError, match="gcc_queue_enqueue"):
            contrast(qd, kd)
        torch.testing.assert_close(cpu(contrast.memory), mem, rtol=0, atol=0)
        return
    ref_mem = mem.clone()
    out_ref, idx_ref = E.moco_forward(ref_mem, index0, qo, k, 0.07)
    loss_ref = E.nce_softmax_loss(out_ref)
    loss_ref.backward()
    out = contrast(qd, kd)
    close(case, "loss", out.loss, loss_ref.detach(), **SCALAR)
    torch.testing.assert_close(cpu(contrast.memory), ref_mem)
    assert contrast.index == idx_ref
    close(case, "dense logits", out.dense(), out_ref.detach(), **DENSE)
    out.loss.backward()
    close(case, "dq", qd.grad, qo.grad, **DQ)


def check_e2e_golden(S):
    g = GOLD["e2e"]
    case = "E2E golden B 6"
    fq = S.t(g["feat_q"]).requires_grad_(True)
    fk = S.t(g["feat_k"]).requires_grad_(True)
    out = e2e_logits(fq, fk, 0.07, engine=S.engine())
    loss = NCESoftmaxLossNS()(out)
    close(case, "loss", loss, g["loss"], **SCALAR)
    close(case, "prob", out.prob, g["prob"], **SCALAR)
    close(case, "dense logits", out.dense(), g["out"], **DENSE)
    rq = g["feat_q"].clone().requires_grad_(True)
    rk = g["feat_k"].clone().requires_grad_(True)
    E.nce_softmax_loss_ns(rk @ rq.t() / 0.07).backward()
    loss.backward()
    close(case, "d feat_q", fq.grad, rq.grad, **DQ)
    close(case, "d feat_k", fk.grad, rk.grad, **DQ)


def check_ema(S):
    torch.manual_seed(0)
    p, e = torch.randn(1000), torch.randn(1000)
    ref = e * 0.999 + (1 - 0.999) * p
    ed = S.t(e)
    S.engine().ema(ed, S.t(p), 0.999, stream=S.stream())
    close("ema n 1000", "ema", ed, ref, rtol=1e-6, atol=1e-7)


def check_bf16_head(S, B, K):
    """GCC_NCE_BF16 (north_star's throughput mode of the head): q, k and the queue rounded to bf16 on load, products on
    the bf16 matrix instruction, fp32 accumulation / softmax.  (1) It must equal the fp32 oracle evaluated on the rounded
    operands (only the summation order differs) -- loss, dense logits, dq.  (2) Against the unrounded fp32 oracle the
    logits move by <= 2^-8 |q||k| / T each; the test states what that does to the loss at T = 0.07: a few 1e-3
    absolute, so north_star's 1e-3 parity bar holds for the f32 mode only, which stays the default."""
    torch.manual_seed(K)
    q = torch.nn.functional.normalize(torch.randn(B, 64), dim=1)
    k = torch.nn.functional.normalize(torch.randn(B, 64), dim=1)
    mem = E.memory_init(K, 64)
    case = f"MoCo bf16 vs oracle on rounded operands B {B} K {K}"
    # oracle on rounded operands
    qr = bf16_round(q).requires_grad_(True)
    out_r, _ = E.moco_forward(bf16_round(mem), 0, qr, bf16_round(k), 0.07)
    loss_r = E.nce_softmax_loss(out_r)
    loss_r.backward()
    out_f, _ = E.moco_forward(mem.clone(), 0, q.clone(), k, 0.07)
    loss_f = E.nce_softmax_loss(out_f)
    contrast = S.moco(K, 0.07, mem, dtype="bf16")
    qd, kd = S.t(q).requires_grad_(True), S.t(k)
    dense = contrast.logits(qd, kd)
    close(case, "dense logits", dense, out_r.detach(), rtol=1e-5, atol=2e-5)
    out = contrast(qd, kd)
    loss = NCESoftmaxLoss()(out)
    close(case, "loss", loss, loss_r.detach(), rtol=1e-5, atol=2e-6)
    loss.backward()
    close(case, "dq", qd.grad, qr.grad, **DQ)
    torch.testing.assert_close(cpu(contrast.memory[:B]), k)                 # the queue itself stays fp32
    err = abs(float(loss.detach()) - float(loss_f.detach()))
    assert err < 2e-2, err                                                   # bf16 operands at T = 0.07: not a 1e-3 mode
    assert (cpu(dense) - out_f.detach()).abs().max() < 64 * 2.0 ** -8 / 0.07 * 0.2


# ----------------------------------------------------------------------------------- the E2E head at ragged batch sizes
def _e2e_run(S, eng, fq, fk, dloss, st=None):
    """pos_mode 1 with rows = feat_k, columns = feat_q (what _NSLoss does), each call from a workspace of 0xFF bytes
    -> (outs, d feat_k, d feat_q)"""
    B = fq.shape[0]
    st = st if st is not None else S.stream()
    ws, nbytes = poison(eng, B, B, S.device)
    outs = eng.forward(fk, None, fq, T, 1, dense=True, stream=st)
    assert ticket(ws, nbytes) == 0
    poison(eng, B, B, S.device)
    dk = eng.backward(fk, None, fq, T, 1, outs, dloss, stream=st)
    poison(eng, B, B, S.device)
    dq = eng.backward(fq, None, fk, T, 1, outs, dloss, by_mem_row=True, stream=st)
    return outs, dk, dq


def check_e2e_ragged(S, B, dtype="f32", dloss=0.75):
    """The in-batch head (pos_mode 1) and both of its gradients -- d feat_k by query, d feat_q through ``by_mem_row``, whose
    softmax runs over the OTHER view's rows and reads lse by queue row -- against float64 cross_entropy(fk fq^T / T, arange(B))
    with autograd; bf16: the same on bf16-rounded operands.  B > 64 makes several query blocks and, with them, several slices.

    B = 1 is degenerate: the only logit is its own lse, p = 1 and both gradients are exactly zero; what the kernels return is
    coef (exp(l' - lse) - 1) x, where l' (the backward's recomputed logit) and lse (the forward's) are two fp32 evaluations of
    the same 64-term dot product, possibly in different orders (bf16: two different matrix instructions).  The relative
    tolerance has nothing to hold on to and atol 1e-7 is below one rounding of the logit, so the bound comes from the formats,
    as check_logits_reach_plus_minus_60's does: each evaluation is off by at most 2^-24 (8 A + |l|) with A = sum |fk_d fq_d| / T
    (8 = sqrt(64) roundings of partial sums that A T bounds, one rounding of the division by T), so |l' - lse| <= 2^-23 (8 A + |l|);
    expf near 1 adds 2^-23 of its own; times the largest term |coef| max |x| = dloss / (B T) max |x|.  Every other batch size
    keeps rtol 1e-4 / atol 1e-7."""
    fq, fk, _ = unit_inputs(B, 1, 4000 + B)
    case = f"E2E {dtype} B {B}"
    eng = S.engine(dtype)
    outs, dk, dq = _e2e_run(S, eng, S.t(fq), S.t(fk), S.t(torch.tensor([dloss], dtype=torch.float32)))
    rnd = bf16_round if dtype == "bf16" else (lambda x: x)
    rq, rk = rnd(fq).double().requires_grad_(True), rnd(fk).double().requires_grad_(True)
    logits = rk @ rq.t() / T
    loss = E.nce_softmax_loss_ns(logits)
    (dloss * loss).backward()
    logits = logits.detach()
    close(case, "loss", outs["loss"].double(), loss.detach(), **SCALAR)
    close(case, "prob", outs["prob"].double(), logits.diagonal().mean(), **SCALAR)
    close(case, "lse", outs["lse"].double(), torch.logsumexp(logits, dim=1), **SCALAR)
    close(case, "pos", outs["pos"].double(), logits.diagonal(), **SCALAR)
    close(case, "dense logits", outs["out"].double(), logits, rtol=1e-5, atol=2e-5 if dtype == "bf16" else 1e-5)
    assert torch.isfinite(cpu(dk)).all() and torch.isfinite(cpu(dq)).all()
    if B == 1:
        A = float((rq.detach() * rk.detach()).abs().sum()) / T
        x = max(float(rq.detach().abs().max()), float(rk.detach().abs().max()))
        bound = dloss / (B * T) * (2.0 ** -23 * (8 * A + float(logits.abs().max())) + 2.0 ** -23) * x
        within(case, "d feat_k", dk, rk.grad, bound)
        within(case, "d feat_q", dq, rq.grad, bound)
        return
    close(case, "d feat_k", dk.double(), rk.grad, **DQ)
    close(case, "d feat_q", dq.double(), rq.grad, **DQ)


# ------------------------------------------------------------------------------------------------------ bits and call order
def _moco_run(S, eng, q, k, mem, dl, one_pass, st=None, fresh_workspace=True):
    """-> [loss, prob, lse, pos, dq] of the one-pass call or of the four launches"""
    B, K = q.shape[0], mem.shape[0]
    st = st if st is not None else S.stream()
    if fresh_workspace:
        poison(eng, B, K, S.device)
    if one_pass:
        outs, dq = eng.forward_backward(q, k, mem, T, dl, stream=st)
    else:
        outs = eng.forward(q, k, mem, T, 0, stream=st)
        if fresh_workspace:
            poison(eng, B, K, S.device)
        dq = eng.backward(q, k, mem, T, 0, outs, dl, stream=st)
    return [outs[n] for n in OUTS] + [dq]


def _e2e_list(S, eng, fq, fk, dl, st=None):
    outs, dk, dq = _e2e_run(S, eng, fq, fk, dl, st)
    return [outs[n] for n in OUTS] + [dk, dq]


def _same_bits(a, b, what):
    names = OUTS + ("dq", "dq by_mem_row")
    for name, x, y in zip(names, a, b):
        assert torch.equal(bits(x), bits(y)), f"{what}: {name} differs in its bits"


def check_identical_calls_give_identical_bits(S, B, K):
    """nce.hip's fixed-order claims: slabs in slice order, the means by the workgroup that arrives last in index order -- two
    identical calls give identical bits in loss, prob, lse, pos and dq (one-pass, four launches, E2E)"""
    q, k, mem = (S.t(x) for x in unit_inputs(B, K, 31 * B + K))
    dl = S.t(torch.tensor([0.75], dtype=torch.float32))
    for one_pass in (True, False):
        eng = S.engine()
        _same_bits(_moco_run(S, eng, q, k, mem, dl, one_pass), _moco_run(S, eng, q, k, mem, dl, one_pass),
                   f"B {B} K {K} {'one-pass' if one_pass else 'four launches'}")
    eng = S.engine()
    _same_bits(_e2e_list(S, eng, q, k, dl), _e2e_list(S, eng, q, k, dl), f"E2E B {B}")


def check_interleaved_calls_on_one_engine(S):
    """(5, 7) and (5, 30) plan to one slice each and to the same workspace byte count, so one engine hands both the same buffer:
    one-pass and four-launch calls of the two shapes interleaved on it, each starting from what the other left behind, equal
    the results of a fresh engine bit for bit"""
    shapes = {name: tuple(S.t(x) for x in unit_inputs(B, K, 100 + K)) for name, (B, K) in (("a", (5, 7)), ("b", (5, 30)))}
    dl = S.t(torch.tensor([0.75], dtype=torch.float32))
    fresh = {(name, one_pass): _moco_run(S, S.engine(), *shapes[name], dl, one_pass, fresh_workspace=False)
             for name in shapes for one_pass in (True, False)}
    eng = S.engine()
    wa, wb = eng._workspace(5, 7, S.device), eng._workspace(5, 30, S.device)
    assert wa[1] == wb[1] and wa[0] is wb[0]
    assert not torch.equal(bits(fresh["a", True][4]), bits(fresh["b", True][4]))
    for name, one_pass in (("a", True), ("b", False), ("a", False), ("b", True), ("a", True), ("b", True), ("b", False), ("a", False)):
        got = _moco_run(S, eng, *shapes[name], dl, one_pass, fresh_workspace=False)
        _same_bits(got, fresh[name, one_pass], f"shape {name}, {'one-pass' if one_pass else 'four launches'}, interleaved")
    assert len(eng._ws) == 1


def check_side_stream_gives_the_default_streams_bits(S, B=70, K=200):
    """device tier only: the calls on a non-default stream (torch.cuda.stream + the engine's stream= argument)"""
    assert S.device.type == "cuda"
    q, k, mem = (S.t(x) for x in unit_inputs(B, K, 31 * B + K))
    dl = S.t(torch.tensor([0.75], dtype=torch.float32))
    default = [_moco_run(S, S.engine(), q, k, mem, dl, True), _moco_run(S, S.engine(), q, k, mem, dl, False),
               _e2e_list(S, S.engine(), q, k, dl)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=S.device)
    assert side.cuda_stream != torch.cuda.current_stream(S.device).cuda_stream
    with torch.cuda.stream(side):
        st = side.cuda_stream
        got = [_moco_run(S, S.engine(), q, k, mem, dl, True, st=st), _moco_run(S, S.engine(), q, k, mem, dl, False, st=st),
               _e2e_list(S, S.engine(), q, k, dl, st=st)]
        side.synchronize()
    for a, b, what in zip(got, default, ("one-pass", "four launches", "E2E")):
        _same_bits(a, b, f"{what} on a side stream")


# -------------------------------------------------------------------------------------------------------- the optimizer tail
def _f32(x):
    """a hyper-parameter as the C ABI receives it (a float argument)"""
    return float(torch.tensor(x, dtype=torch.float32))


def _scratch_ticket(scratch):
    return cpu(scratch).view(torch.int32)[2:4].tolist()


def check_adam(S, n, tail=None):
    """gcc_adam_step (``tail`` None: gradnorm_kernel + tail_norm_kernel<0>) or gcc_adam_ema_step with n_ema = n + tail (the EMA copy
    covers ``tail`` elements past the live prefix) over two steps, the first with the gradient norm above max_norm 1.0, the
    second below it, against a float64 restatement of clip_grad_norm_ + torch.optim.Adam (L2 weight decay) + moment_update
    (train.py:169-172,409,417).  The restatement takes lr, the betas, eps, the weight decay and the EMA momentum at the float
    values the C ABI receives.  Parameters, the clipped gradient left in ``grad``, the returned norm and the EMA copy at Adam's
    tolerance; the scratch ticket back at 0 after every call."""
    lr, b1, b2, eps, wd, m_ema = (_f32(x) for x in (0.005, 0.9, 0.999, 1e-8, 1e-5, 0.999))
    n_all = n + (tail or 0)
    gen = torch.Generator().manual_seed(41 * n + (tail or 0))
    flat0, ema0 = torch.randn(n_all, generator=gen), torch.randn(n_all, generator=gen)
    case = f"adam n {n}" if tail is None else f"adam_ema n {n} tail {tail}"
    eng, st = S.engine(), S.stream()
    flat, ema = S.t(flat0), S.t(ema0)
    param = flat[:n]
    grad, m, v = (S.t(torch.zeros(n)) for _ in range(3))
    gn, scratch = S.t(torch.zeros(1)), S.t(torch.zeros(64, dtype=torch.float64))
    rp, re, rm, rv = flat0.double().clone(), ema0.double().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step, scale in ((1, 3.0), (2, 0.5)):
        u = torch.randn(n, generator=gen)
        g = u / u.norm() * scale
        grad.copy_(S.t(g))
        if tail is None:
            eng.adam(param, grad, m, v, 0.005, (0.9, 0.999), 1e-8, 1e-5, step, 1.0, gn, scratch, stream=st)
        else:
            eng.adam_ema(param, grad, m, v, 0.005, (0.9, 0.999), 1e-8, 1e-5, step, 1.0, gn, scratch, stream=st, ema=ema, ema_src=flat,
                         ema_m=0.999)
        assert _scratch_ticket(scratch) == [0, 0]
        # clip_grad_norm_(max_norm = 1)
        rg = g.double()
        norm = rg.pow(2).sum().sqrt()
        assert (float(norm) > 1.0) == (step == 1)
        rg = rg * torch.clamp(1.0 / (norm + 1e-6), max=1.0)
        # torch.optim.Adam
        gi = rg + wd * rp[:n]
        rm = b1 * rm + (1 - b1) * gi
        rv = b2 * rv + (1 - b2) * gi * gi
        denom = rv.sqrt() / (1 - b2 ** step) ** 0.5 + eps
        rp[:n] = rp[:n] - lr / (1 - b1 ** step) * rm / denom
        re = re * m_ema + (1 - m_ema) * rp            # moment_update
        close(case, f"step {step} grad norm", gn.double().reshape(()), norm, **ADAM)
        close(case, f"step {step} clipped gradient", grad.double(), rg, **ADAM)
        close(case, f"step {step} parameters", param.double(), rp[:n], **ADAM)
        if tail is not None:
            close(case, f"step {step} EMA copy", ema.double(), re, **ADAM)
            assert torch.equal(cpu(flat[n:]), flat0[n:])                            # past the live prefix: only averaged


def check_ema_ragged(S, n):
    """gcc_ema_update against float64 p2 * m + (1 - m) * p1 (moment_update) with m at its float value; check_ema's tolerance"""
    gen = torch.Generator().manual_seed(n)
    p, e = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m = _f32(0.999)
    ed = S.t(e)
    S.engine().ema(ed, S.t(p), 0.999, stream=S.stream())
    close(f"ema n {n}", "ema", ed.double(), e.double() * m + (1 - m) * p.double(), rtol=1e-6, atol=1e-7)


# ---------------------------------------------------------------------------------------------------------------- the enqueue
def check_enqueue(S):
    """gcc_queue_enqueue with as many keys as the queue has rows, and from index K - 1 (the wrap comes right after the first
    key): the saved rows are the rows that were overwritten, the queue holds the keys at (index + i) mod K and nothing else
    moved; more keys than rows are refused with rc -1 and leave the queue alone"""
    eng, st = S.engine(), S.stream()
    for K, nkeys, index in ((48, 48, 16), (48, 48, 0), (200, 200, 199), (48, 6, 47), (200, 70, 199), (1, 1, 0)):
        gen = torch.Generator().manual_seed(K + nkeys + index)
        mem0, keys = torch.randn(K, 64, generator=gen), torch.randn(nkeys, 64, generator=gen)
        mem = S.t(mem0)
        saved = eng.enqueue(mem, S.t(keys), index, save=True, stream=st)
        rows = (index + torch.arange(nkeys)) % K
        assert torch.equal(cpu(saved), mem0[rows]), (K, nkeys, index)
        expect = mem0.clone()
        expect[rows] = keys
        assert torch.equal(cpu(mem), expect), (K, nkeys, index)
        mem = S.t(mem0)
        assert eng.enqueue(mem, S.t(keys), index, save=False, stream=st) is None
        assert torch.equal(cpu(mem), expect), (K, nkeys, index)
    K = 48
    mem0 = torch.randn(K, 64, generator=torch.Generator().manual_seed(9))
    mem, keys = S.t(mem0), S.t(torch.ones(K + 1, 64))
    assert S.lib.gcc_queue_enqueue(S.ptr(mem), K, S.ptr(keys), K + 1, 0, None, st) == -1
    assert "gcc_queue_enqueue" in S.lib.gcc_last_error().decode()
    assert torch.equal(cpu(mem), mem0)
