"""ProNE on the device against the reference's library calls on the host -> profiles/prone_probe.json.

    python tools/prone_probe.py [--reps 5] [--shapes airport hindex bench] [--out profiles/prone_probe.json]

Per shape (Chung-Lu graphs of gcc_amd.graphgen with the sizes of usa_airport, of the h-index corpus and of the bench graph; d = 64):
  device_ms      ``ProNEEngine.embed`` from host arrays to the status read: the draw and upload of Omega, the CSR upload, every
                 kernel.  Median of ``reps`` after one warm-up call.
  omega_ms       the host draw of Omega and its upload alone (part of device_ms), and its share.
  host_ms        tests/prone_reference.embed_library on the same host: sklearn's randomized_svd, scipy's sparse products and
                 scipy.linalg.svd, with whatever thread count the environment sets (reported).  ``host_reps`` runs, median.
  stages         GPU time of single stage calls, events around each, in a run of their own (no counters, no tracing): the node
                 terms, one product F X and one M X with the HALF tail at their widths, one orthonormalisation at k = 74.
  spmm           for the F X product: bytes by two models over the time and over the HBM peak.  ``frac``: the compulsory
                 bytes (x read once, y written once, row_ptr, col_idx, r, c).  ``frac_moved``: what the kernel asks for (one row
                 of x per neighbour, nnz k 8 bytes, whatever cache it comes from, plus the same writes and indices).
Nothing here is asserted; where the host wins, the JSON says so (``device_over_host`` > 1)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcc_amd import _cabi  # noqa: E402
from gcc_amd.graphgen import powerlaw_graph  # noqa: E402
from gcc_amd.prone import ProNEEngine, draw_omega  # noqa: E402
from tests import prone_reference as R  # noqa: E402

PEAK_HBM_GBS = 8000.0
SHAPES = {"airport": (1190, 27200, 5), "hindex": (5000, 88000, 5), "bench": (1_000_000, 10_000_000, 1)}      # nodes, entries, host reps


def gpu_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def probe(name, reps, d=64):
    nodes, entries, host_reps = SHAPES[name]
    row_ptr, col_idx = powerlaw_graph(nodes, entries, 0)
    n, nnz, k = len(row_ptr) - 1, len(col_idx), d + _cabi.PRONE_OVERSAMPLE
    eng = ProNEEngine(device="cuda:0")
    dev = eng.device

    def whole():
        res = eng.embed(row_ptr, col_idx, d, seed=0)
        eng.check_status(res)
        return res

    whole()
    device_ms = wall_ms(whole, reps)
    omega_ms = wall_ms(lambda: (torch.from_numpy(draw_omega(n, d, 0)).to(dev), torch.cuda.synchronize()), reps)
    host_ms = wall_ms(lambda: R.embed_library(row_ptr, col_idx, d, seed=0), host_reps)
    # ---- single stage calls
    rp, ci = torch.from_numpy(row_ptr).to(dev), torch.from_numpy(col_idx).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    x, y = torch.randn(n, k, dtype=torch.float64, device=dev), torch.empty(n, k, dtype=torch.float64, device=dev)
    xd, yd, zd, cv = (torch.randn(n, d, dtype=torch.float64, device=dev) for _ in range(4))

    def stage(call, **members):
        a, keep, _ = eng.graph_args(rp, ci, d)
        for key, v in members.items():
            setattr(a, key, eng.ptr(v) if isinstance(v, torch.Tensor) else v)
        return lambda: eng.call(call, a, status)

    stages = dict(
        node_terms_ms=gpu_ms(stage("gcc_prone_node_terms"), reps),
        spmm_f_k74_ms=gpu_ms(stage("gcc_prone_spmm", mode=_cabi.PRONE_MODE_F, k=k, x=x, y=y), reps),
        spmm_m_half_d64_ms=gpu_ms(stage("gcc_prone_spmm", mode=_cabi.PRONE_MODE_M, tail=_cabi.PRONE_TAIL_HALF, k=d, mu=0.2, alpha=1.0,
                                        beta=-0.5, x=xd, z=zd, y=yd, conv=cv), reps),
        orthonormalize_k74_ms=gpu_ms(stage("gcc_prone_orthonormalize", k=k, y=x.clone()), reps))
    assert int(status.cpu()[0]) == 0
    compulsory = 2 * n * k * 8 + 4 * (nnz + n + 1) + 2 * 8 * n
    moved = nnz * k * 8 + n * k * 8 + 4 * (nnz + n + 1) + 8 * (nnz + n)
    sec = stages["spmm_f_k74_ms"] * 1e-3
    spmm = dict(bytes_compulsory=compulsory, bytes_moved=moved, gbs=compulsory / sec / 1e9, gbs_moved=moved / sec / 1e9,
                frac=compulsory / sec / 1e9 / PEAK_HBM_GBS, frac_moved=moved / sec / 1e9 / PEAK_HBM_GBS)
    return dict(shape=name, n=n, nnz=nnz, d=d, max_degree=int(np.diff(row_ptr).max()), device_ms=device_ms, omega_ms=omega_ms,
                omega_share=omega_ms / device_ms, host_ms=host_ms, host_reps=host_reps, device_over_host=device_ms / host_ms,
                stages=stages, spmm=spmm)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prone_probe.json"))
    a = ap.parse_args()
    results = []
    for shape in a.shapes:
        results.append(probe(shape, a.reps))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, peak_hbm_gbs=PEAK_HBM_GBS,
                       host_threads=os.environ.get("OMP_NUM_THREADS"), results=results), f, indent=1)
