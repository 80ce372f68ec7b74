"""The one-pass MoCo head (gcc_nce_forward_backward: nce_onepass_kernel + nce_merge_kernel of gcc_amd/csrc/nce.hip) on the
wave64 emulator against the four-launch head (gcc_nce_forward + gcc_nce_backward) and against a float64 restatement in
torch: loss, prob, lse, pos, dq.  Tolerances are tests/test_nce_emu.py's for this head."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from gcc_amd.contrast import NceEngine
from tests.hipemu.emu_driver import emu_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 0.07


class _Recorder:
    """the emulator library with the names of the C-ABI calls made through it"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._lib, name)


def emu_nce(dtype="f32", record=False):
    lib = emu_lib()
    return NceEngine(lib=_Recorder(lib) if record else lib, ptr=lambda t: 0 if t is None else t.data_ptr(), dtype=dtype)


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


def check_case(q, k, mem, dloss=1.0, patch=None, patch_index=0, T=T, dq_bound=None):
    """one-pass == float64 reference == four launches, each at the head's tolerances (``dq_bound``: see
    test_logits_reach_plus_minus_60)"""
    eng = emu_nce()
    dl = torch.tensor([dloss], dtype=torch.float32)
    outs, dq = eng.forward_backward(q, k, mem, T, dl, patch=patch, patch_index=patch_index)
    old = eng.forward(q, k, mem, T, 0, patch=patch, patch_index=patch_index)
    dq_old = eng.backward(q, k, mem, T, 0, old, dl, patch=patch, patch_index=patch_index)
    ref = reference_f64(q, k, mem, dloss, patch, patch_index, T)
    for name in ("loss", "prob"):
        torch.testing.assert_close(outs[name].double().reshape(()), ref[name], rtol=1e-5, atol=1e-6, msg=lambda m: f"{name}: {m}")
        torch.testing.assert_close(outs[name], old[name], rtol=1e-5, atol=1e-6, msg=lambda m: f"{name} vs four launches: {m}")
    for name in ("lse", "pos"):
        torch.testing.assert_close(outs[name].double(), ref[name], rtol=1e-5, atol=1e-6, msg=lambda m: f"{name}: {m}")
        torch.testing.assert_close(outs[name], old[name], rtol=1e-5, atol=1e-6, msg=lambda m: f"{name} vs four launches: {m}")
    assert torch.isfinite(dq).all()
    if dq_bound is not None:
        err, err_old = (dq.double() - ref["dq"]).abs().max(), (dq_old.double() - ref["dq"]).abs().max()
        print(f"dq: largest error {float(err):.3e} (four launches {float(err_old):.3e}), bound {dq_bound:.3e}")
        assert err <= dq_bound and err_old <= dq_bound
        return outs, dq
    torch.testing.assert_close(dq.double(), ref["dq"], rtol=1e-4, atol=1e-7, msg=lambda m: f"dq: {m}")
    torch.testing.assert_close(dq_old.double(), ref["dq"], rtol=1e-4, atol=1e-7, msg=lambda m: f"dq of the four launches: {m}")
    return outs, dq


def unit_inputs(B, K, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=1)
    k = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=1)
    mem = torch.nn.functional.normalize(torch.randn(K, 64, generator=g), dim=1)
    return q, k, mem


# K = 100: two slices, the last one 36 rows (shorter than a 64-row chunk); K = 4097: the last slice is ONE row (B <= 64: 65
# slices of 64 rows -- past the merge kernel's first 64 --, B = 65: 128-row slices, B = 256: 33 slices of 128); K = 200 at
# B > 64: slices of 64 rows with a last one of 8
@pytest.mark.parametrize("K", [64, 100, 200, 4097])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 256])
def test_onepass_head_shapes(B, K):
    check_case(*unit_inputs(B, K, 1000 * B + K))


def test_more_than_64_slices_by_workgroup_count():
    """GCC_NCE_WGS = 512 (read once per process: a process of its own): K = 8197, B = 8 -> 129 slices of 64 rows, the last of 5;
    the merge kernel's loop over slice blocks runs three times"""
    code = ("import torch, tests.test_nce_onepass_emu as t\n"
            "eng = t.emu_nce()\n"
            "assert eng.lib.gcc_nce_workspace_bytes(8, 8197) > 129 * 8 * 64 * 4\n"      # (129 slabs: the plan did take the setting)
            "t.check_case(*t.unit_inputs(8, 8197, 5), dloss=0.5)\n")
    env = dict(os.environ, GCC_NCE_WGS="512", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def _quantised(B, K, seed, scale):
    """operands on a dyadic grid (q, k: 1 / 16; queue: 1 / 8) and T = 1 / 16: every logit is EXACT in fp32"""
    q, k, _ = unit_inputs(B, K, seed)
    g = torch.Generator().manual_seed(seed + 1)
    mem = torch.round(torch.randn(K, 64, generator=g) * scale * 8) / 8
    return torch.round(q * 16) / 16, torch.round(k * 16) / 16, mem


@pytest.mark.parametrize("B,K", [(5, 300), (70, 1000)])
def test_logits_reach_plus_minus_60(B, K):
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
    check_case(q, k, mem, T=T16)
    check_case(q, k, mem, T=T16, dloss=0.25)
    q, k, _ = unit_inputs(B, K, 7 * B + K)                        # (b)
    mem = torch.randn(K, 64, generator=torch.Generator().manual_seed(K)) * 1.5
    logits = torch.cat([q @ mem.t(), 3.0 * (q * k).sum(1, keepdim=True)], 1) / T
    assert logits.max() > 60 and logits.min() < -60
    bound = 9 * 2.0 ** -24 * float(logits.abs().max()) / (B * T) * float(mem.abs().max())
    check_case(q, 3.0 * k, mem, dq_bound=bound)                   # (a positive logit far above 1 / T as well)


@pytest.mark.parametrize("order", ["increasing", "decreasing"])
def test_monotonic_maximum_along_the_queue(order):
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
    check_case(q, k, mem)


def test_lane_groups_of_a_query_need_one_common_maximum():
    """rows 4 g .. 4 g + 3 of every 16-row tile belong to lane group g: with the large logits in ONE lane group's rows only, a
    maximum kept per lane group would weigh the other groups' rows by their own (much smaller) maxima"""
    B, K = 17, 128
    q, k, mem = unit_inputs(B, K, 11)
    big = (torch.arange(K) % 16) // 4 == 2
    mem = torch.where(big[:, None], mem, 0.05 * mem)        # (unit rows at most: the regime the tolerances were set in)
    check_case(q, k, mem)


def test_patch_rows_and_dloss():
    B, K = 70, 200
    q, k, mem = unit_inputs(B, K, 13)
    g = torch.Generator().manual_seed(17)
    patch = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=1)
    outs, dq = check_case(q, k, mem, dloss=-2.5, patch=patch, patch_index=170)      # wraps: rows 170..199, 0..39
    _, dq1 = check_case(q, k, mem, dloss=1.0, patch=patch, patch_index=170)
    torch.testing.assert_close(dq, -2.5 * dq1, rtol=1e-6, atol=0)
    _, dq0 = check_case(q, k, mem)
    assert not torch.equal(dq1, dq0)                                               # (the patch is really read)


def test_bf16_keeps_the_four_launches():
    """the one-pass kernels are f32; --nce-dtype bf16 stays on gcc_nce_forward + gcc_nce_backward, and the library refuses it"""
    B, K = 6, 48
    q, k, mem = unit_inputs(B, K, 19)
    eng = emu_nce("bf16", record=True)
    assert not eng.one_pass()
    dl = torch.ones(1)
    outs, dq = eng.forward_backward(q, k, mem, T, dl)
    assert "gcc_nce_forward_backward" not in eng.lib.calls and {"gcc_nce_forward", "gcc_nce_backward"} <= set(eng.lib.calls)
    old = eng.forward(q, k, mem, T, 0)
    assert torch.equal(dq, eng.backward(q, k, mem, T, 0, old, dl)) and torch.equal(outs["loss"], old["loss"])
    f32 = emu_nce(record=True)
    f32.forward_backward(q, k, mem, T, dl)
    assert "gcc_nce_forward_backward" in f32.lib.calls and "gcc_nce_backward" not in f32.lib.calls
    a = eng._args(q, k, mem, 1.0 / T, 0, None, 0, outs, None)
    assert a.dtype == 1
    ws, nbytes = eng._workspace(B, K, q.device)
    rc = emu_lib().gcc_nce_forward_backward(ctypes.byref(a), dl.data_ptr(), dq.data_ptr(), ws.data_ptr(), nbytes, None, None, None)
    assert rc == -2
