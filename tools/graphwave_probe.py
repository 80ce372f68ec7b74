"""GraphWave on the device against its float64 NumPy restatement on the same host -> profiles/graphwave_probe.json.

    python tools/graphwave_probe.py [--reps 5] [--shapes airport hindex panther] [--host-limit-s 240] [--out profiles/graphwave_probe.json]

Per shape (Chung-Lu graphs of gcc_amd.graphgen with the sizes of usa_airport and of the h-index corpus, and a panther-sized
multigraph: a third of its edges carry 2 or 3 parallel copies; d = 64):
  device_ms      ``GraphWaveEngine.embed`` from host arrays to the status read: the host's coefficients, the CSR upload, every
                 kernel.  Median of ``reps`` wall-clock runs after one warm-up call.
  gpu_ms         the same call's GPU time alone, events around it (the arrays already on the device).
  host_ms        ``gcc_amd.graphwave.embed_numpy`` (what ``--device cpu`` serves: scipy's sparse products on dense panels, NumPy's
                 cos / sin), one run, with whatever thread count the environment sets (reported).  A shape whose run is expected
                 to exceed ``--host-limit-s`` (the previous shape's time scaled by the square of the node counts) is skipped and
                 ``host_skipped`` says so.
  panels         GPU time of gcc_graphwave_heat per panel (the node scales, orders 0 and 1, the 29 gather products with both heat
                 sums, the thresholded write-out), summed over the panels.
  step           the gather products' rate over those calls: 29 nnz W 8 bytes of gathered neighbour rows per panel over the
                 panels' time (a lower bound: the calls hold more than the products), beside the 1.6 TB/s that prone.hip's
                 product reached with the same access pattern.
  char_share     1 - panels / gpu_ms: the share of the call in the characteristic pass and the table (a lower bound by the same
                 argument: the heat calls' write-out is not part of ``embed``).
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
from gcc_amd.graphwave import GraphWaveEngine, embed_numpy  # noqa: E402
from gcc_amd.ingest import multigraph_csr  # noqa: E402

PRONE_GATHER_GBS = 1600.0
SHAPES = {"airport": (1190, 27200, False), "panther": (2800, 22000, True), "hindex": (5000, 88000, False)}      # nodes, entries, multigraph


def graph(name):
    nodes, entries, multi = SHAPES[name]
    row_ptr, col_idx = powerlaw_graph(nodes, entries, 0)
    if multi:
        rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
        keep = rows < col_idx
        pairs = np.stack([rows[keep], col_idx[keep]], axis=1)
        weights = np.random.RandomState(0).choice([1, 1, 1, 1, 2, 3], size=len(pairs))
        row_ptr, col_idx = multigraph_csr(pairs, weights, len(row_ptr) - 1)
    return row_ptr, col_idx


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


def probe(name, reps, host_limit_s, previous, d=64):
    row_ptr, col_idx = graph(name)
    n, nnz = len(row_ptr) - 1, len(col_idx)
    eng = GraphWaveEngine(device="cuda:0")
    dev = eng.device

    def whole():
        res = eng.embed(row_ptr, col_idx, d)
        eng.check_status(res)
        return res

    chi = whole()["chi"].cpu().numpy()
    device_ms = wall_ms(whole, reps)
    rp, ci = torch.from_numpy(row_ptr).to(dev), torch.from_numpy(col_idx).to(dev)
    gpu = gpu_ms(lambda: eng.embed(rp, ci, d), reps)
    width = eng.panel_width(n, d)
    chunks = (n + width - 1) // width
    panels = sum(gpu_ms(lambda c=c: eng.heat(rp, ci, d, chunk=c), reps) for c in range(chunks))
    gathered = (_cabi.GRAPHWAVE_ORDER - 1) * nnz * n * 8
    out = dict(shape=name, n=n, nnz=nnz, d=d, max_degree=int(np.diff(row_ptr).max()), panel_width=int(width), panels=chunks,
               device_ms=device_ms, gpu_ms=gpu, panels_ms=panels, char_share=1.0 - panels / gpu,
               step=dict(gathered_bytes=gathered, gbs=gathered / (panels * 1e-3) / 1e9, prone_gbs=PRONE_GATHER_GBS))
    expected = previous["host_ms"] * 1e-3 * (n / previous["n"]) ** 2 if previous else 0.0
    if expected > host_limit_s:
        out.update(host_ms=None, host_skipped=f"expected {expected:.0f} s from the previous shape, above the limit of {host_limit_s} s")
        return out
    t0 = time.perf_counter()
    ref = embed_numpy(row_ptr, col_idx, d)["chi"]
    host_ms = (time.perf_counter() - t0) * 1e3
    out.update(host_ms=host_ms, host_reps=1, device_over_host=device_ms / host_ms, max_abs_difference=float(np.abs(chi - ref).max()))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--host-limit-s", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "graphwave_probe.json"))
    a = ap.parse_args()
    results, previous = [], None
    for shape in a.shapes:
        results.append(probe(shape, a.reps, a.host_limit_s, previous))
        if results[-1].get("host_ms"):
            previous = results[-1]
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, host_threads=os.environ.get("OMP_NUM_THREADS"), results=results),
                  f, indent=1)
