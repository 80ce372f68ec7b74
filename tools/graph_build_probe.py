"""The device build of the contract CSR (gcc_graph_build) and the device contract check (gcc_graph_check) against the host routes,
on one MI355X -> profiles/graph_build_probe.json.

    python tools/graph_build_probe.py [--reps 5] [--shapes g1 hub g2] [--host-reps-large 1] [--kernel-stats] [--out profiles/graph_build_probe.json]

Per shape, on the SAME raw lines (seeded; ids drawn with a power-law density and scattered over the id range, self loops and repeats
as they fall; ``hub``: one node on 150,000 lines besides):
  device_ms        ``GraphBuildEngine.build`` from the host array to the sliced CSR: the upload of ``pairs``, every kernel and the
                   one host read (``counts``).  Median of ``reps`` wall-clock runs after one warm-up call.
  gpu_ms           the same call with ``pairs`` already on the device, device events around it (the read of ``counts`` ends it).
  reference_ms     the reference converter's own route on the host: both directions of the lines that are no self loop,
                   ``sp.coo_matrix(...).tocsr()``, the degree filter and the relabel (``sort_indices`` included: DGL hands out
                   sorted rows).
  numpy_ms         the route of ``gcc_amd.graphgen._powerlaw_graph`` from its ``src != dst`` line on (``np.unique`` of the
                   undirected keys, the relabel, two sorts).
                   Host routes: median of ``reps`` runs, of ``--host-reps-large`` above 20 M lines (said in ``host_reps``), with
                   whatever thread count the environment sets.  Both are checked to give the device's CSR bit for bit.
  check            on the graph just built (g1, g2): ``gcc_graph_check`` with the CSR on the device to the status read (``device_ms``;
                   ``upload_ms``: what ``DeviceGraph(validate="device")`` spends before it and the host check does not) against
                   ``graphgen.check_contract`` (``host_ms``).
  *_over_device    host time over device time: above 1 the device wins, below 1 it loses.
``--kernel-stats``: additionally ONE run of its own under ``rocprofv3 --kernel-trace --stats`` per shape (this script with
``--child``), the kernels' total times from its statistics file, and for the scatter and the compact kernels the bytes the
algorithm moves (from the shapes: scatter 8 m + 24 x inserted lines -- the lines, two row starts, two cursor atomics and two slots
per line; compact 12 x entries + 24 n -- slot, new id and the written column per entry, six words per node) over the kernel's time
as a fraction of the HBM peak (8.0 TB/s; a float4 copy reaches 6.29).  Nothing here is asserted; losses stay in the JSON."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcc_amd.graph_build import GraphBuildEngine  # noqa: E402
from gcc_amd.graphgen import _chunked, check_contract  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = {"g1": (1_000_000, 5_000_000, 0), "hub": (300_000, 1_000_000, 150_000), "g2": (10_000_000, 100_000_000, 0)}   # n, lines, hub lines
LARGE = 20_000_000


def lines_of(name):
    n, m, hub = SHAPES[name]
    rng = np.random.Generator(np.random.PCG64(len(name) + n))
    perm = rng.permutation(n).astype(np.int32)
    pairs = np.empty((m + hub, 2), dtype=np.int32)
    for col in range(2):
        pairs[:m, col] = perm[np.minimum((n * rng.random(m) ** 2.5).astype(np.int64), n - 1)]
    if hub:
        pairs[m:, 0] = perm[0]
        pairs[m:, 1] = rng.integers(0, n, hub)
        pairs = rng.permutation(pairs, axis=0)
    return n, np.ascontiguousarray(pairs)


def reference_route(pairs, n):
    import scipy.sparse as sp

    u, v = pairs[:, 0], pairs[:, 1]
    keep = u != v
    u, v = u[keep], v[keep]
    row, col = np.concatenate([u, v]), np.concatenate([v, u])
    a = sp.coo_matrix((np.ones(len(row), dtype=np.int32), (row, col)), shape=(n, n)).tocsr()
    a.sort_indices()
    alive = np.diff(a.indptr) > 0
    new = (np.cumsum(alive) - 1).astype(np.int32)
    row_ptr = np.zeros(int(alive.sum()) + 1, dtype=np.int64)
    np.cumsum(np.diff(a.indptr)[alive], out=row_ptr[1:])
    return row_ptr.astype(np.int32), new[a.indices]


def numpy_route(pairs, n):
    """gcc_amd.graphgen._powerlaw_graph from the line that drops the self loops on"""
    src, dst = pairs[:, 0], pairs[:, 1]
    keep = src != dst
    src, dst = src[keep], dst[keep]
    lo, hi = np.minimum(src, dst).astype(np.int64), np.maximum(src, dst).astype(np.int64)
    key = np.unique(lo * n + hi)
    lo, hi = key // n, key % n
    deg = np.bincount(lo, minlength=n) + np.bincount(hi, minlength=n)
    alive = deg > 0
    relabel = np.cumsum(alive) - 1
    v = int(alive.sum())
    lo, hi = relabel[lo], relabel[hi]
    back = hi * v + lo
    back.sort()
    keys = np.concatenate([lo * v + hi, back])
    del lo, hi, back, key
    keys.sort(kind="stable")
    rows = np.concatenate(_chunked(lambda a, b: keys[a:b] // v, len(keys)))
    cols = np.concatenate(_chunked(lambda a, b: (keys[a:b] - rows[a:b] * v).astype(np.int32), len(keys)))
    row_ptr = np.zeros(v + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=v), out=row_ptr[1:])
    return row_ptr.astype(np.int32), cols


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def event_ms(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def probe(name, reps, host_reps_large):
    n, pairs = lines_of(name)
    m = len(pairs)
    eng = GraphBuildEngine(device="cuda:0")
    res = eng.build(pairs, n)                                       # (warm-up; also the result the host routes are held against)
    eng.check_status(res)
    rp, ci, counts = res["row_ptr"].cpu().numpy(), res["col_idx"].cpu().numpy(), [int(c) for c in res["counts"]]
    out = dict(shape=name, n=n, lines=m, counts=dict(zip(("nodes", "entries", "self_loop_lines", "duplicate_slots", "zero_degree_nodes",
                                                          "max_degree"), counts)))
    out["device_ms"] = wall_ms(lambda: eng.build(pairs, n), reps)
    resident = torch.from_numpy(pairs).to("cuda:0")
    out["gpu_ms"] = event_ms(lambda: eng.build(resident, n), reps)
    out["workspace_bytes"] = int(eng.workspace(0).numel())
    host_reps = reps if m <= LARGE else host_reps_large
    out["host_reps"] = host_reps
    for key, route in (("reference_ms", reference_route), ("numpy_ms", numpy_route)):
        times = []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            got = route(pairs, n)
            times.append((time.perf_counter() - t0) * 1e3)
        out[key] = statistics.median(times)
        out[key.replace("_ms", "_same_bits")] = bool(np.array_equal(got[0], rp) and np.array_equal(got[1], ci))
        del got
        out[key.replace("_ms", "_over_device")] = out[key] / out["device_ms"]
    if name != "hub":
        chk = dict(upload_ms=wall_ms(lambda: (torch.from_numpy(rp).to("cuda:0"), torch.from_numpy(ci).to("cuda:0"), torch.cuda.synchronize()), reps))
        eng.validate(res["row_ptr"], res["col_idx"])
        chk["device_ms"] = wall_ms(lambda: eng.validate(res["row_ptr"], res["col_idx"]), reps)
        chk["host_ms"] = wall_ms(lambda: check_contract(rp, ci), host_reps)
        chk["host_over_device"] = chk["host_ms"] / chk["device_ms"]
        chk["host_over_device_with_upload"] = chk["host_ms"] / (chk["device_ms"] + chk["upload_ms"])
        out["check"] = chk
    return out


def child(name):
    """what the kernel-statistics run executes: one warm-up and one counted build and check"""
    n, pairs = lines_of(name)
    eng = GraphBuildEngine(device="cuda:0")
    for _ in range(2):
        res = eng.build(pairs, n)
        eng.validate(res["row_ptr"], res["col_idx"])
    torch.cuda.synchronize()


def kernel_stats(name, result):
    """-> {kernel: ms per call} of one rocprofv3 run of ``child(name)`` (two calls of everything), plus the two byte rates"""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "gb", "--", sys.executable, os.path.abspath(__file__),
               "--child", name]
        run = subprocess.run(cmd, capture_output=True, text=True)
        found = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if run.returncode != 0 or not found:
            return dict(error=f"rocprofv3 exit {run.returncode}, {len(found)} statistics files", stderr=run.stderr[-400:])
        rows = list(csv.DictReader(open(found[0])))
    per = {}
    for r in rows:
        short = [k for k in r["Name"].replace("(", " ").replace(":", " ").split() if k.endswith("_kernel")]
        if short and short[0][:3] in ("gb_", "gc_"):
            per[short[0]] = per.get(short[0], 0.0) + float(r["TotalDurationNs"]) / 2 * 1e-6       # (two counted calls)
    c = result["counts"]
    inserted = result["lines"] - c["self_loop_lines"]
    out = dict(ms_per_call=per, total_ms=sum(per.values()))
    for kernels, nbytes, key in ((("gb_scatter_kernel",), 8 * result["lines"] + 24 * inserted, "scatter"),
                                 (("gb_compact_kernel", "gb_compact_large_kernel"), 12 * c["entries"] + 24 * result["n"], "compact")):
        ms = sum(per.get(k, 0.0) for k in kernels)
        if ms:
            out[key] = dict(bytes=nbytes, ms=ms, tb_per_s=nbytes / (ms * 1e-3) / 1e12, fraction_of_hbm_peak=nbytes / (ms * 1e-3) / HBM_PEAK)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--host-reps-large", type=int, default=1)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--child", default=None, choices=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "graph_build_probe.json"))
    a = ap.parse_args()
    if a.child:
        child(a.child)
        sys.exit(0)
    if not torch.cuda.is_available():
        sys.exit("graph_build_probe.py measures on the GPU: none found")
    results = []
    for shape in a.shapes:
        results.append(probe(shape, a.reps, a.host_reps_large))
        if a.kernel_stats:
            results[-1]["kernels"] = kernel_stats(shape, results[-1])
        print(json.dumps(results[-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                                 # (after every shape: a later one may run out of time)
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, host_threads=os.environ.get("OMP_NUM_THREADS"),
                           hbm_peak_tb_per_s=HBM_PEAK / 1e12, results=results), f, indent=1)
