"""Records the emulator's pos / evals / raw bit patterns for SIMPLE graphs -- stalky_view(), dense_views() and
_sampled_views(160, 10, 11) of tests/test_posemb_emu.py, default switches -- into tests/golden/posemb_simple_bits.npz.
The dense classes' matrix assembly counts parallel edges (repeated CSR entries); a run of one entry must write the very
float it wrote before, so these outputs may not move by a bit.  Run this at the commit BEFORE a change of the
assembly, from the repository root (python -m tests.golden.make_posemb_simple_golden)."""
import os

import numpy as np

from tests import test_posemb_emu as T

SWITCHES = ("GCC_POSEMB_CHEB", "GCC_POSEMB_PAIR", "GCC_POSEMB_WAVE", "GCC_POSEMB_STALKS")     # recorded at their defaults


def views():
    """name -> view, in the order the golden file holds them"""
    out = {"stalky": T.stalky_view()[0]}
    for i, v in enumerate(T.dense_views()):
        out["dense%d" % i] = v
    out["sampled"] = T._sampled_views(160, 10, 11)
    return out


if __name__ == "__main__":
    for name in SWITCHES:
        os.environ.pop(name, None)
    rec = {}
    for name, view in views().items():
        x, evals, raw = T._run(view)
        for key, arr in (("pos", x), ("evals", evals), ("raw", raw)):
            rec["%s_%s" % (name, key)] = np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32)
    path = os.path.join(os.path.dirname(__file__), "posemb_simple_bits.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in rec.items()})
