"""DeviceGraph construction three ways on one MI355X -> profiles/graph_tables_probe.json.

    python tools/graph_tables_probe.py [--reps 5] [--shapes g1 hub g2] [--host-reps-large 1] [--kernel-stats] [--out profiles/graph_tables_probe.json]

Per shape of tools/graph_build_probe.py (the same seeded lines, built by gcc_graph_build first; g1: 1 M nodes / 10 M entries, hub: the
hub-heavy file, g2: 10 M / 200 M), wall clock from the call to the finished object, uploads and host reads included, median of
``reps`` runs after one warm-up (``--host-reps-large`` runs for the two routes with host work above 20 M entries, said in
``host_reps``):
  host_ms           ``DeviceGraph(row_ptr, col_idx, validate=True)`` from the arrays on the host: the host check, the host tables, the
                    uploads -- the only route before gcc_graph_check existed.
  device_check_ms   ``DeviceGraph(..., validate="device")``: upload, the check on the device, the tables on the host.
  from_device_ms    ``DeviceGraph.from_device(row_ptr, col_idx, validate="device")`` on the CSR where gcc_graph_build left it: the check
                    and the tables on the device (gcc_graph_tables), two host reads (status, summary), the upload of ``ltab``.
  tables_ms         the table build alone (``GraphTablesEngine.tables``: both calls and the summary read), device events around it.
  same_integers     the three objects agree in every integer attribute and table (the cdf differs in its last bits by design);
  cdf_units         the device cdf's largest distance from the exact cdf (np.longdouble) in units of 2^-53, and the host's.
``--kernel-stats``: additionally ONE run of its own under ``rocprofv3 --kernel-trace --stats`` per shape (this script with
``--child``): the gt_* and gc_* kernels' times per call.  Nothing here is asserted; a shape where the host wins stays in the JSON."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from graph_build_probe import SHAPES, lines_of  # noqa: E402

from gcc_amd.graph import DeviceGraph  # noqa: E402
from gcc_amd.graph_build import GraphBuildEngine  # noqa: E402
from gcc_amd.graph_tables import GraphTablesEngine  # noqa: E402

LARGE = 20_000_000
INTEGERS = ("num_nodes", "num_edges", "max_degree", "sb_degree", "lmax", "num_hubs", "hub_words", "contract_checked", "max_copies")
TENSORS = ("row_ptr", "col_idx", "ltab", "hub_index", "hub_adj")


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        del keep
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


def same_integers(a, b):
    for name in INTEGERS:
        if getattr(a, name) != getattr(b, name):
            return False
    for name in TENSORS:
        x, y = getattr(a, name), getattr(b, name)
        if (x is None) != (y is None) or (x is not None and not torch.equal(x, y)):
            return False
    return True


def cdf_units(cdf, rp):
    w = np.diff(rp).astype(np.longdouble) ** np.longdouble(0.75)
    exact = np.cumsum(w) / w.sum()
    return float(np.abs(cdf.astype(np.longdouble) - exact).max()) * 2.0 ** 53


def built(name):
    n, pairs = lines_of(name)
    eng = GraphBuildEngine(device="cuda:0")
    res = eng.build(pairs, n)
    eng.check_status(res)
    return res


def probe(name, reps, host_reps_large):
    res = built(name)
    rp_d, ci_d = res["row_ptr"].clone(), res["col_idx"].clone()
    rp, ci = rp_d.cpu().numpy(), ci_d.cpu().numpy()
    del res
    out = dict(shape=name, nodes=len(rp) - 1, entries=len(ci))
    host_reps = reps if len(ci) <= LARGE else host_reps_large
    out["host_reps"] = host_reps
    dev = DeviceGraph.from_device(rp_d, ci_d, validate="device")                 # (warm-up, and the object the others are held against)
    out.update(max_degree=dev.max_degree, num_hubs=dev.num_hubs, hub_adj_bytes=int(dev.hub_adj.numel() * 4) if dev.hub_adj is not None else 0)
    out["from_device_ms"] = wall_ms(lambda: DeviceGraph.from_device(rp_d, ci_d, validate="device"), reps)
    teng = GraphTablesEngine(device="cuda:0")
    teng.tables(rp_d, ci_d)
    out["tables_ms"] = event_ms(lambda: teng.tables(rp_d, ci_d), reps)
    mid = DeviceGraph(rp, ci, device="cuda:0", validate="device")
    out["device_check_ms"] = wall_ms(lambda: DeviceGraph(rp, ci, device="cuda:0", validate="device"), host_reps)
    host = DeviceGraph(rp, ci, device="cuda:0", validate=True)
    out["host_ms"] = wall_ms(lambda: DeviceGraph(rp, ci, device="cuda:0", validate=True), host_reps)
    out["same_integers"] = bool(same_integers(dev, host) and same_integers(mid, host))
    out["cdf_units"] = dict(device=cdf_units(dev.seed_cdf.cpu().numpy(), rp), host=cdf_units(host.seed_cdf.cpu().numpy(), rp))
    out["host_over_from_device"] = out["host_ms"] / out["from_device_ms"]
    out["device_check_over_from_device"] = out["device_check_ms"] / out["from_device_ms"]
    return out


def child(name):
    """what the kernel-statistics run executes: one warm-up and one counted construction"""
    res = built(name)
    for _ in range(2):
        DeviceGraph.from_device(res["row_ptr"], res["col_idx"], validate="device")
    torch.cuda.synchronize()


def kernel_stats(name):
    """-> {kernel: ms per call} of one rocprofv3 run of ``child(name)`` (two calls of everything)"""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "gt", "--", sys.executable, os.path.abspath(__file__),
               "--child", name]
        run = subprocess.run(cmd, capture_output=True, text=True)
        found = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if run.returncode != 0 or not found:
            return dict(error=f"rocprofv3 exit {run.returncode}, {len(found)} statistics files", stderr=run.stderr[-400:])
        rows = list(csv.DictReader(open(found[0])))
    per = {}
    for r in rows:
        short = [k for k in r["Name"].replace("(", " ").replace(":", " ").split() if k.endswith("_kernel")]
        if short and short[0][:3] in ("gt_", "gc_"):
            per[short[0]] = per.get(short[0], 0.0) + float(r["TotalDurationNs"]) / 2 * 1e-6       # (two counted calls)
    return dict(ms_per_call=per, total_ms=sum(per.values()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--host-reps-large", type=int, default=1)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--child", default=None, choices=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_tables_probe.json"))
    a = ap.parse_args()
    if a.child:
        child(a.child)
        sys.exit(0)
    if not torch.cuda.is_available():
        sys.exit("graph_tables_probe.py measures on the GPU: none found")
    results = []
    for shape in a.shapes:
        results.append(probe(shape, a.reps, a.host_reps_large))
        if a.kernel_stats:
            results[-1]["kernels"] = kernel_stats(shape)
        print(json.dumps(results[-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                                 # (after every shape: a later one may run out of time)
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, host_threads=os.environ.get("OMP_NUM_THREADS"), results=results),
                      f, indent=1)
