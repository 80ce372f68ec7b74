"""One SHA-256 per output array of the downstream-task kernels (ProNE, GraphWave, logistic regression, SVC, similarity search) on
the check modules' fixtures, from ANY build of the library: run it on two builds and compare the files line by line.

    python tools/downstream_bits.py --lib gcc_amd/csrc/libgcc_amd.so --out bits_device.txt
    python tools/downstream_bits.py --lib tests/hipemu/_build/libgcc_amd_emu.so --emu --out bits_emu.txt

The library goes in through the engines' ``lib`` seam; ``--emu``: CPU tensors and plain addresses (the emulator build), else
cuda:0.  The emulator's hashes depend on the host's libm: compare them between builds on one machine only."""
import argparse
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcc_amd import _cabi  # noqa: E402
from tests import graphwave_check, logreg_check, prone_check, simsearch_check, svc_check  # noqa: E402
from tests import graphwave_reference, prone_reference  # noqa: E402


def cases(lib, ptr, device, emu):
    """-> (case name, dict of arrays) one by one"""
    pr = prone_check.Pr(lib, ptr, device)
    for name in ["n201d16", "n300d6", "n40d2", "hub"] + ([] if emu else ["n120d64", "n74d64"]):
        for chunk in (0, 32, prone_check.SPLIT_CHUNK):
            yield f"prone {name} chunk {chunk}", pr.embed(prone_reference.fixture(name), chunk=chunk)
    gw = graphwave_check.Gw(lib, ptr, device)
    for name in ("n257d64", "hub300d8", "multi130d32", "n40d256"):
        fx = graphwave_reference.fixture(name)
        for width in (0, 64):
            yield f"graphwave {name} width {width}", gw.embed(fx["row_ptr"], fx["col_idx"], fx["d"], width=width)
    fx = graphwave_reference.fixture("n65d8")
    yield "graphwave heat n65d8", gw.heat(fx["row_ptr"], fx["col_idx"], fx["d"])
    lr = logreg_check.Lr(lib, ptr, device)
    for name in ["sep", "d1", "t15", "t16", "t17", "stride"] + ([] if emu else ["c128", "c129"]):
        fx = logreg_check.fixture(name)
        yield f"logreg {name}", lr.fit(fx["X"], fx["y"], fx["fold"], extra=fx["extra"], C=logreg_check.C, tol=logreg_check.TOL)
    svc = svc_check.Svc(lib, ptr, device)
    for name in ("a", "m3", "w"):                # a binary and a multiclass case, and the four-wave kernel's shape
        fx = svc_check.fixtures()[name]
        yield f"svc {name}", svc.fit(fx["X"], fx["y"], fx["fold"], C=fx["C"])
    sim = simsearch_check.Sim(lib, ptr, device)
    for name in simsearch_check.CASES:
        for tier in ("exact", "norm"):
            yield f"simsearch {name} {tier}", sim.search(simsearch_check.problem(name, tier))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", required=True, help="libgcc_amd.so or the emulator build of it")
    ap.add_argument("--emu", action="store_true", help="the library is the emulator build: CPU tensors")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    lib = _cabi.declare(ctypes.CDLL(os.path.abspath(a.lib)))      # (torch is imported: its HIP runtime is the process's)
    ptr = (lambda t: t.data_ptr() if t is not None else None) if a.emu else _cabi.dev_ptr
    lines = []
    for case, arrays in cases(lib, ptr, "cpu" if a.emu else "cuda:0", a.emu):
        for key in sorted(arrays):
            if isinstance(arrays[key], np.ndarray):
                v = np.ascontiguousarray(arrays[key])
                lines.append(f"{hashlib.sha256(v.tobytes()).hexdigest()}  {case}: {key} {v.dtype}{list(v.shape)}")
        print(case, flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
