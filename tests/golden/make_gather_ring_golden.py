"""Records what the gather cases of tests/gather_ring_check.py give into tests/golden/gather_ring_bits_<tier>.npz, tier = emu
(the wave64 emulator) or gpu (the device; the two contract differently).  A change of gather_tile that moves requests and no
addition must reproduce them bit for bit, so run this on the library of the commit BEFORE such a change, from the root of a
checkout that has the tests (``library``: that commit's libgcc_amd_emu.so / libgcc_amd.so; default: this checkout's own):
    python -m tests.golden.make_gather_ring_golden emu|gpu [library [output path]]
Every case is run twice and must repeat itself: the statistics are sums of fp64 atomics, the recording holds only what does
not depend on their order."""
import ctypes
import sys

import numpy as np

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
    for name, (view, hint, kind) in K.cases().items():
        a, b = (K.record(name, K.run_case(T, name, view, hint, kind)) for _ in range(2))
        for k in a:
            assert np.array_equal(a[k], b[k]), (name, k, "does not repeat itself")
            out["%s__%s" % (name, k)] = a[k]
        print(name, sorted(a))
    path = sys.argv[3] if len(sys.argv) > 3 else K.golden_path(tier)
    np.savez_compressed(path, **out)
    import os

    print(path, os.path.getsize(path), "bytes")
