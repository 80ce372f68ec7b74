"""Records what the cases of tests/head_means_check.py give in the ticket mode into tests/golden/head_means_bits_<tier>.npz,
tier = emu (the wave64 emulator) or gpu (the device).  A change of the head that moves work and changes no addition must
reproduce them bit for bit, so run this on the library of the commit BEFORE such a change, from the root of a checkout that has
the tests (``library``: that commit's libgcc_amd_emu.so / libgcc_amd.so; default: this checkout's own):
    python -m tests.golden.make_head_means_golden emu|gpu [library [output path]]
Every case is run twice and must repeat itself.  The case of 129 slices runs in a child process (GCC_NCE_WGS is read once)."""
import os
import subprocess
import sys

import numpy as np

from tests import head_means_check as C


def _record(S, name, case, wgs=256):
    a, b = (C.run_case(S, case, False, wgs=wgs) for _ in range(2))
    for k in a:
        assert np.array_equal(a[k], b[k]), (name, k, "does not repeat itself")
    print(name, sorted(a))
    return {"%s__%s" % (name, k): v for k, v in a.items()}


if __name__ == "__main__":
    tier = sys.argv[1]
    assert tier in ("emu", "gpu")
    library = sys.argv[2] if len(sys.argv) > 2 else ""
    path = sys.argv[3] if len(sys.argv) > 3 else C.golden_path(tier)
    S = C.head_of(tier, library)
    if os.environ.get("GCC_NCE_WGS") == "512":          # the child: the one case of 129 slices
        assert C.plan(8, 8197, 512)[0] == 129
        np.savez_compressed(path, **_record(S, C.MANY_SLICES[0], C.MANY_SLICES[1], wgs=512))
        sys.exit(0)
    out = {}
    for name, case in C.cases().items():
        out.update(_record(S, name, case))
    child = path + ".many.npz"
    subprocess.run([sys.executable, "-m", "tests.golden.make_head_means_golden", tier, library, child], check=True,
                   env=dict(os.environ, GCC_NCE_WGS="512"), cwd=C.ROOT)
    out.update(dict(np.load(child)))
    os.remove(child)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
