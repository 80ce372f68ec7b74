"""The four-launch MoCo head (gcc_nce_forward + gcc_nce_backward, gcc_amd/csrc/nce.hip) with its two means formed where the
caller chooses, for both tiers (tests/test_head_means_emu.py: the wave64 emulator; tests/test_head_means_gpu.py: the device).

In the ticket mode (pos_mode 0) nce_combine_kernel's last workgroup forms loss / prob behind an arrival counter; in the deferred
mode (GCC_NCE_POS_MOCO_DEFERRED) the forward call ends with lse / pos and one extra workgroup of nce_dq_kernel forms them, by the
same device function.  No addition differs, so in BOTH modes every case must give the bits that the commit before wrote on the
same tier in the only mode it had (tests/golden/head_means_bits_<tier>.npz, tests/golden/make_head_means_golden.py): the
per-slice maxima and sums pm / ps, lse, pos, loss, prob, the dq slabs and dq.  Arrays of more than 1024 words are recorded as
their first 1024 words and two 64-bit checksums over all of them (the slabs of the largest case are 1 MiB).

Cases: B in {1, 63, 65, 256} x K in {17, 64, 65, 1000} in f32 (K = 65: a last slice of one row), four of them in bf16, patch
rows that wrap round the queue's end, and 129 slices (GCC_NCE_WGS = 512, read once per process: a child process).  Every call
starts from a workspace of 0xFF bytes and must leave the arrival counter at 0; the deferred forward call must leave loss / prob
alone."""
import os
import subprocess
import sys

import numpy as np
import torch

from tests import nce_check as N

ROOT = N.ROOT
T = 0.07
DLOSS = 0.75
SENTINEL = -123.0
HEAD = 1024


def cases():
    """name -> (B, K, dtype, patch rows, patch index)"""
    out = {}
    for B in (1, 63, 65, 256):
        for K in (17, 64, 65, 1000):
            out["b%d_k%d_f32" % (B, K)] = (B, K, "f32", 0, 0)
    for B, K in ((1, 17), (63, 64), (65, 65), (256, 1000)):
        out["b%d_k%d_bf16" % (B, K)] = (B, K, "bf16", 0, 0)
    out["patch_wraps_f32"] = (63, 200, "f32", 5, 198)          # rows 198, 199, 0, 1, 2
    out["patch_wraps_bf16"] = (63, 200, "bf16", 5, 198)
    return out


MANY_SLICES = ("many_slices_f32", (8, 8197, "f32", 0, 0))       # with GCC_NCE_WGS = 512: 129 slices of 64 rows, the last of 5


def plan(B, K, wgs=256):
    """make_plan of nce.hip: slices, rows per slice, byte offsets of pm / ps / slabs"""
    qb = (B + 63) // 64
    s = max(1, min((wgs + qb - 1) // qb, (K + 63) // 64))
    R = (((K + s - 1) // s) + 63) // 64 * 64
    S = (K + R - 1) // R
    al = lambda x: (x + 255) // 256 * 256
    off_ps = al(S * B * 4)
    off_slabs = off_ps + al(S * B * 4)
    return S, R, 0, off_ps, off_slabs


def _words(ws, off, n):
    return ws[off:off + 4 * n].cpu().numpy().copy().view(np.uint32)


def compact(w):
    """an array's words, or (above HEAD words) its first HEAD words and two checksums over all of them"""
    w = np.ascontiguousarray(w).reshape(-1).view(np.uint32)
    if w.size <= HEAD:
        return w
    x = w.astype(np.uint64)
    i = (np.arange(w.size, dtype=np.uint64) % np.uint64(65521)) + np.uint64(1)
    with np.errstate(over="ignore"):
        sums = np.array([x.sum(dtype=np.uint64), (x * i).sum(dtype=np.uint64)], dtype=np.uint64)
    return np.concatenate([w[:HEAD], sums.view(np.uint32)])


def run_case(S, case, deferred, wgs=256):
    """-> dict of uint32 arrays; asserts what every call must leave behind"""
    B, K, dtype, prow, pidx = case
    q, k, mem = N.unit_inputs(B, K, 7000 + 13 * B + K)
    patch = None
    if prow:
        patch = torch.nn.functional.normalize(torch.randn(prow, 64, generator=torch.Generator().manual_seed(9)), dim=1)
    q, k, mem, patch = S.t(q), S.t(k), S.t(mem), S.t(patch)
    dl = S.t(torch.tensor(DLOSS))
    eng = S.engine(dtype)
    st = S.stream()
    ws, nbytes = N.poison(eng, B, K, S.device)
    kw = dict(patch=patch, patch_index=pidx, stream=st)
    if deferred:
        kw["defer_means"] = True
    outs = eng.forward(q, k, mem, T, 0, **kw)
    if S.device.type == "cuda":
        torch.cuda.synchronize()
    assert N.ticket(ws, nbytes) == 0, "the forward call leaves the arrival counter at 0"
    Sn, R, off_pm, off_ps, off_slabs = plan(B, K, wgs)
    assert S.lib.gcc_nce_workspace_bytes(B, K) == off_slabs + (Sn * B * 64 * 4 + 255) // 256 * 256 + 256, "the plan"
    res = {"pm": _words(ws, off_pm, Sn * B), "ps": _words(ws, off_ps, Sn * B)}
    if deferred:                                   # loss / prob are the backward call's to write: whatever they hold now goes
        outs["loss"].fill_(SENTINEL)
        outs["prob"].fill_(SENTINEL)
    else:
        res["loss_fwd"], res["prob_fwd"] = (N.bits(outs[x]).numpy().view(np.uint32).copy() for x in ("loss", "prob"))
        outs["loss"].fill_(SENTINEL)               # ... and the ticket mode's backward call must NOT write them
        outs["prob"].fill_(SENTINEL)
    dq = eng.backward(q, k, mem, T, 0, outs, dl, **kw)
    if S.device.type == "cuda":
        torch.cuda.synchronize()
    assert N.ticket(ws, nbytes) == 0, "the backward call leaves the arrival counter at 0"
    loss, prob = float(outs["loss"][0]), float(outs["prob"][0])
    if deferred:
        assert loss != SENTINEL and prob != SENTINEL, "the deferred backward call forms the means"
        res["loss"], res["prob"] = (N.bits(outs[x]).numpy().view(np.uint32).copy() for x in ("loss", "prob"))
    else:
        assert loss == SENTINEL and prob == SENTINEL, "the ticket mode's backward call leaves the means alone"
        res["loss"], res["prob"] = res.pop("loss_fwd"), res.pop("prob_fwd")
    res["lse"], res["pos"] = (N.bits(outs[x]).numpy().view(np.uint32).copy() for x in ("lse", "pos"))
    res["slabs"] = compact(_words(ws, off_slabs, Sn * B * 64))
    res["dq"] = compact(N.bits(dq).numpy())
    # the means are what they are called: float64 over the recorded lse / pos.  prob: the fp64 mean rounded once to f32
    # (2^-24 of it); loss: that, and each lse - pos was rounded to f32 before it was summed (2^-24 of the largest).
    lse, pos = (res[x].view(np.float32).astype(np.float64) for x in ("lse", "pos"))
    want_l, want_p = float((lse - pos).mean()), float(pos.mean())
    got_l, got_p = (float(res[x].view(np.float32)[0]) for x in ("loss", "prob"))
    assert abs(got_l - want_l) <= 2.0 ** -24 * 1.001 * (abs(want_l) + np.abs(lse - pos).max()), (got_l, want_l)
    assert abs(got_p - want_p) <= 2.0 ** -24 * 1.001 * abs(want_p), (got_p, want_p)
    return res


def deferred_forward_leaves_the_means_alone(S):
    """through the argument struct: loss / prob preset, the deferred forward call does not touch them"""
    import ctypes

    B, K = 65, 200
    q, k, mem = (S.t(x) for x in N.unit_inputs(B, K, 3))
    eng = S.engine("f32")
    f32 = dict(dtype=torch.float32, device=S.device)
    outs = dict(lse=torch.empty(B, **f32), pos=torch.empty(B, **f32), loss=torch.full((1,), SENTINEL, **f32),
                prob=torch.full((1,), SENTINEL, **f32))
    ws, nbytes = N.poison(eng, B, K, S.device)
    a = eng._args(q, k, mem, 1.0 / T, eng.MOCO_DEFERRED, None, 0, outs, None)
    rc = S.lib.gcc_nce_forward(ctypes.byref(a), S.ptr(ws), nbytes, None, S.stream())
    assert rc == 0
    if S.device.type == "cuda":
        torch.cuda.synchronize()
    assert float(outs["loss"][0]) == SENTINEL and float(outs["prob"][0]) == SENTINEL
    assert N.ticket(ws, nbytes) == 0
    assert torch.isfinite(outs["lse"]).all() and torch.isfinite(outs["pos"]).all()
    # a dense output, the E2E diagonal and the one-pass pair have no deferred form
    dense = torch.empty(B, K + 1, **f32)
    a = eng._args(q, k, mem, 1.0 / T, eng.MOCO_DEFERRED, None, 0, outs, dense)
    assert S.lib.gcc_nce_forward(ctypes.byref(a), S.ptr(ws), nbytes, None, S.stream()) != 0
    a = eng._args(q, k, mem, 1.0 / T, eng.MOCO_DEFERRED, None, 0, outs, None)
    dq, dl = torch.empty_like(q), S.t(torch.tensor([1.0]))
    assert S.lib.gcc_nce_backward(ctypes.byref(a), S.ptr(dl), 1, S.ptr(dq), S.ptr(ws), nbytes, None, S.stream()) != 0
    assert S.lib.gcc_nce_forward_backward(ctypes.byref(a), S.ptr(dl), S.ptr(dq), S.ptr(ws), nbytes, None, None, S.stream()) != 0


def head_of(tier, library=None):
    """the tier's head on this checkout's library, or on the library at ``library`` (the recording)"""
    if not library:
        return N.head(tier)
    import ctypes

    from gcc_amd import _cabi

    lib = _cabi.declare(ctypes.CDLL(library))
    return N.Head(lib, N.emu_ptr, "cpu") if tier == "emu" else N.Head(lib, _cabi.dev_ptr, "cuda:0")


def golden_path(tier):
    return os.path.join(os.path.dirname(__file__), "golden", "head_means_bits_%s.npz" % tier)


def compare(name, res, z):
    for key, v in res.items():
        w = z["%s__%s" % (name, key)]
        assert v.shape == w.shape and np.array_equal(v, w), (name, key, int((v != w).sum()), "words differ")


def check_case(S, tier, name):
    z = np.load(golden_path(tier))
    ticket, deferred = run_case(S, cases()[name], False), run_case(S, cases()[name], True)
    assert sorted(ticket) == sorted(deferred)
    compare(name, ticket, z)
    compare(name, deferred, z)


def check_many_slices(tier):
    """GCC_NCE_WGS = 512 is read once per process: both modes in a child process, against the recording"""
    name = MANY_SLICES[0]
    code = ("import numpy as np\n"
            "from tests import head_means_check as C, nce_check as N\n"
            f"S = N.head({tier!r})\n"
            "assert C.plan(8, 8197, 512)[0] == 129\n"
            f"z = np.load(C.golden_path({tier!r}))\n"
            "for deferred in (False, True):\n"
            f"    C.compare({name!r}, C.run_case(S, C.MANY_SLICES[1], deferred, wgs=512), z)\n")
    env = dict(os.environ, GCC_NCE_WGS="512", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


def check_cases_are_what_they_are_named_for():
    S, R = plan(8, 65)[:2]
    assert (S, R) == (2, 64) and 65 - (S - 1) * R == 1            # K = 65: a last slice of one row
    assert plan(256, 1000)[0] == 16 and plan(8, 8197, 512)[0] == 129
    B, K, _, prow, pidx = cases()["patch_wraps_f32"]
    assert pidx + prow > K                                          # the patch wraps round the queue's end
