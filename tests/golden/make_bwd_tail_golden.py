"""Records what the cases of tests/bwd_tail_check.py give into tests/golden/bwd_tail_bits_<tier>.npz, tier = emu (the wave64
emulator) or gpu (the device; the two contract differently).  A change of gin_bwd_emb_kernel or gin_grad_final_kernel that moves
requests or spreads work and changes no addition must reproduce them bit for bit; a change that does re-order a sum records
anew, on the library of the commit BEFORE it or its own, from the root of a checkout that has the tests (``library``: that commit's libgcc_amd_emu.so /
libgcc_amd.so; default: this checkout's own):
    python -m tests.golden.make_bwd_tail_golden emu|gpu [library [output path]]
Every case is run twice and must repeat itself."""
import ctypes
import os
import sys

import numpy as np

from tests import bwd_tail_check as C
from tests import gather_ring_check as K

if __name__ == "__main__":
    tier = sys.argv[1]
    assert tier in ("emu", "gpu")
    lib = None
    if len(sys.argv) > 2 and sys.argv[2]:
        from gcc_amd import _cabi

        lib = _cabi.declare(ctypes.CDLL(sys.argv[2]))
    T = K.Tier(tier, lib)
    out = {}
    for name in C.cases():
        a, b = (C.record(C.run_case(T, name)) for _ in range(2))
        for k in a:
            assert np.array_equal(a[k], b[k]), (name, k, "does not repeat itself")
            out["%s__%s" % (name, k)] = a[k]
        print(name, sorted(a))
    path = sys.argv[3] if len(sys.argv) > 3 else C.golden_path(tier)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
