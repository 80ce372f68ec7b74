"""Records the pos / evals / raw bit patterns of the sparse block class's build cases (tests/posemb_block_build_cases.py)
into tests/golden/posemb_block_build_bits_<tier>.npz, tier = emu (the wave64 emulator) or gpu (the device).  A change of
posemb_cheb_kernel that reorders work without changing one arithmetic operation must reproduce them bit for bit, so run
this at the commit BEFORE such a change, from the repository root:
    python -m tests.golden.make_posemb_block_build_golden emu|gpu [output path]"""
import os
import sys

import numpy as np

from tests import posemb_block_build_cases as K


def run(tier, view, hidden):
    """-> pos, evals, raw, status words of one case on ``tier``"""
    import torch

    from gcc_amd.posemb import DevicePosEmb

    if tier == "emu":
        from tests.hipemu.emu_driver import emu_lib
        from tests.hipemu.emu_encoder import CpuBatch

        b = CpuBatch(dict(view, pos_undirected=torch.zeros(int(view["node_off"][-1]), hidden)))
        pe = DevicePosEmb(b.batch_size, b.parent_nid.numel(), hidden, device="cpu", lib=emu_lib(),
                          ptr=lambda t: 0 if t is None else t.data_ptr())
        evals, raw = torch.zeros(b.batch_size, hidden), torch.zeros(b.parent_nid.numel(), hidden)
        pe(b, evals=evals, raw=raw)
        return b.pos_undirected.numpy(), evals.numpy(), raw.numpy(), [int(v) for v in pe.status]
    from gcc_amd.sampler import BatchedCSR

    no, rp, ci = (view[k].numpy() for k in ("node_off", "row_ptr", "col_idx"))
    B, n = len(no) - 1, int(no[-1])
    q = BatchedCSR(B, torch.from_numpy(no.astype(np.int32)).cuda(), torch.from_numpy(rp[no].astype(np.int32)).cuda(),
                   torch.zeros(n, dtype=torch.int32, device="cuda"),
                   torch.from_numpy(np.repeat(np.arange(B), np.diff(no)).astype(np.int32)).cuda(),
                   torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(ci.astype(np.int32)).cuda())
    q.pos_undirected = torch.zeros(n, hidden, device="cuda")
    pe = DevicePosEmb(B, n, hidden, device="cuda", seed=7)
    evals, raw = torch.zeros(B, hidden, device="cuda"), torch.zeros(n, hidden, device="cuda")
    pe(q, evals=evals, raw=raw)
    pe.check_status(strict=True)
    return q.pos_undirected[:n].cpu().numpy(), evals.cpu().numpy(), raw[:n].cpu().numpy(), [int(v) for v in pe.status.cpu()]


def golden_path(tier):
    return os.path.join(os.path.dirname(__file__), "posemb_block_build_bits_%s.npz" % tier)


if __name__ == "__main__":
    tier = sys.argv[1]
    assert tier in ("emu", "gpu")
    for name in ("GCC_POSEMB_CHEB", "GCC_POSEMB_PAIR", "GCC_POSEMB_WAVE", "GCC_POSEMB_STALKS"):    # recorded at their defaults
        os.environ.pop(name, None)
    rec = {}
    for name, (view, hidden, _) in K.cases().items():
        x, evals, raw, status = run(tier, view, hidden)
        print(name, "status", status)
        for key, arr in (("pos", x), ("evals", evals), ("raw", raw)):
            rec["%s_%s" % (name, key)] = K.bits(arr)
    path = sys.argv[2] if len(sys.argv) > 2 else golden_path(tier)
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")
