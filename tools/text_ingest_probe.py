"""The device reader of ``.lscc`` text (gcc_text_line_ends / gcc_text_ints, gcc_amd.text_ingest) against the host reader
(``ingest.read_lscc``), each from the file's path to the finished ``gcc_graph_build`` output, on one MI355X
-> profiles/text_ingest_probe.json.

    python tools/text_ingest_probe.py [--reps 5] [--shapes g1 hub [g2]] [--kernel-stats] [--out profiles/text_ingest_probe.json]

Per shape a seeded file of the lines of ``tools/graph_build_probe.py`` (``n`` vertex lines, then ``u v 1`` per line) is written to a
temporary folder and read once (page cache).  After one warm-up of each route the two routes ALTERNATE in this process, ``reps``
times; every figure is the median, wall clock, milliseconds:
  host    read_lscc_ms   ``ingest.read_lscc(path)``
          build_ms       ``GraphBuildEngine.build`` of its array (upload, kernels, the read of ``counts``)
          total_ms       both
  device  total_ms       ``TextIngestEngine.read_lscc(path)`` and ``GraphBuildEngine.build`` of its device tensor, as a user runs them
          build_ms       the build alone (in the same run)
          upload_ms, calls_ms, host_reads_ms   a second set of ``reps`` runs with a device synchronisation after every stage, so
                         that the stages can be told apart: the file read and the chunked copy; gcc_text_line_ends and gcc_text_ints
                         to their completion; the three host reads (the two line ends, the ``<word> m`` line, the summary)
  host_over_device       host total_ms over device total_ms: above 1 the device wins, below 1 it loses.
``g2`` (10 M nodes / 100 M lines) runs only when asked for and when the host has 48 GB available for the host route; otherwise the
JSON says that it was not run.
``--kernel-stats``: additionally ONE run of its own under ``rocprofv3 --kernel-trace --stats`` per shape (this script with
``--child``): the ti_* kernels' time per call, and for the count and the parse pass the bytes they move (count: the text; parse: the
body and the 8 m bytes of pairs) over that time as a fraction of the HBM peak (8.0 TB/s; a float4 copy reaches 6.29).  Nothing here
is asserted; losses stay in the JSON."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gcc_amd import ingest  # noqa: E402
from gcc_amd.graph_build import GraphBuildEngine  # noqa: E402
from gcc_amd.text_ingest import TextIngestEngine  # noqa: E402
from graph_build_probe import HBM_PEAK, SHAPES, lines_of  # noqa: E402

G2_HOST_BYTES = 48 << 30


def write_file(name, path):
    """-> (n, lines, the file's bytes, the bytes of its edge lines)"""
    n, pairs = lines_of(name)
    with open(path, "wb") as f:
        f.write(b"vertices %d\n" % n)
        for at in range(0, n, 1 << 20):
            f.write(b"".join(b"%d %d\n" % (i, i) for i in range(at, min(at + (1 << 20), n))))
        f.write(b"edges %d\n" % len(pairs))
        body_at = f.tell()
        for at in range(0, len(pairs), 1 << 20):
            f.write(b"".join(b"%d %d 1\n" % (u, v) for u, v in pairs[at:at + (1 << 20)].tolist()))
    return n, len(pairs), os.path.getsize(path), os.path.getsize(path) - body_at


def available_bytes():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


class Staged(TextIngestEngine):
    """the engine with a synchronisation and a clock after every stage of read_lscc"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.ms = dict(upload=0.0, calls=0.0)

    def _timed(self, key, fn, *a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a, **k)
        torch.cuda.synchronize()
        self.ms[key] += (time.perf_counter() - t0) * 1e3
        return out

    def _upload(self, *a, **k):
        return self._timed("upload", super()._upload, *a, **k)

    def line_ends(self, *a, **k):
        return self._timed("calls", super().line_ends, *a, **k)

    def ints(self, *a, **k):
        return self._timed("calls", super().ints, *a, **k)


def probe(name, path, reps):
    n, lines, nbytes, body_bytes = write_file(name, path)
    with open(path, "rb") as f:
        while f.read(1 << 24):                                      # (page cache)
            pass
    build, text = GraphBuildEngine(device="cuda:0"), TextIngestEngine(device="cuda:0")
    out = dict(shape=name, n=n, lines=lines, file_bytes=nbytes, body_bytes=body_bytes)

    def host_route():
        t0 = time.perf_counter()
        got_n, pairs = ingest.read_lscc(path)
        t1 = time.perf_counter()
        res = build.build(pairs, got_n)
        t2 = time.perf_counter()
        return dict(read_lscc_ms=(t1 - t0) * 1e3, build_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3), pairs, res

    def device_route(engine=text):
        t0 = time.perf_counter()
        got_n, pairs = engine.read_lscc(path)
        t1 = time.perf_counter()
        res = build.build(pairs, got_n)
        t2 = time.perf_counter()
        return dict(read_lscc_ms=(t1 - t0) * 1e3, build_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3), pairs, res

    _, host_pairs, host_res = host_route()                          # (warm-up of each route; also the two results compared)
    _, dev_pairs, dev_res = device_route()
    out["same_pairs"] = bool(np.array_equal(dev_pairs.cpu().numpy(), host_pairs))
    out["same_csr"] = bool(torch.equal(dev_res["row_ptr"], host_res["row_ptr"]) and torch.equal(dev_res["col_idx"], host_res["col_idx"]))
    out["counts"] = [int(c) for c in dev_res["counts"]]
    del host_pairs, dev_pairs, host_res, dev_res
    host, device = [], []
    for _ in range(reps):
        host.append(host_route()[0])
        device.append(device_route()[0])
    staged = []
    for _ in range(reps):
        eng = Staged(device="cuda:0")
        t0 = time.perf_counter()
        eng.read_lscc(path)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        staged.append(dict(upload_ms=eng.ms["upload"], calls_ms=eng.ms["calls"], host_reads_ms=total - eng.ms["upload"] - eng.ms["calls"],
                           read_lscc_synchronised_ms=total))

    def med(rows):
        return {k: statistics.median(r[k] for r in rows) for k in rows[0]}

    out["host"], out["device"] = med(host), {**med(device), **med(staged)}
    out["host_over_device"] = out["host"]["total_ms"] / out["device"]["total_ms"]
    out["read_lscc_host_over_device"] = out["host"]["read_lscc_ms"] / out["device"]["read_lscc_ms"]
    out["upload_gb_per_s"] = nbytes / (out["device"]["upload_ms"] * 1e-3) / 1e9
    return out


def child(path):
    """what the kernel-statistics run executes: one warm-up and one counted read"""
    eng = TextIngestEngine(device="cuda:0")
    for _ in range(2):
        eng.read_lscc(path)
    torch.cuda.synchronize()


def kernel_stats(path, result):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "ti", "--", sys.executable, os.path.abspath(__file__),
               "--child", path]
        run = subprocess.run(cmd, capture_output=True, text=True)
        found = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if run.returncode != 0 or not found:
            return dict(error=f"rocprofv3 exit {run.returncode}, {len(found)} statistics files", stderr=run.stderr[-400:])
        rows = list(csv.DictReader(open(found[0])))
    per = {}
    for r in rows:
        short = [k for k in r["Name"].replace("(", " ").replace(":", " ").split() if k.endswith("_kernel")]
        if short and short[0].startswith("ti_"):
            per[short[0]] = float(r["TotalDurationNs"]) / max(int(r["Calls"]), 1) * 1e-6
    out = dict(ms_per_call=per)
    for kernel, nbytes, key in (("ti_count_kernel", result["file_bytes"], "count"),
                                ("ti_parse_kernel", result["body_bytes"] + 8 * result["lines"], "parse")):
        ms = per.get(kernel, 0.0)
        if ms:
            out[key] = dict(bytes=nbytes, ms=ms, tb_per_s=nbytes / (ms * 1e-3) / 1e12, fraction_of_hbm_peak=nbytes / (ms * 1e-3) / HBM_PEAK)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["g1", "hub"], choices=list(SHAPES))
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--child", default=None, help="a file to read twice (the kernel-statistics run)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "text_ingest_probe.json"))
    a = ap.parse_args()
    if a.child:
        child(a.child)
        sys.exit(0)
    if not torch.cuda.is_available():
        sys.exit("text_ingest_probe.py measures on the GPU: none found")
    results, not_run = [], {}
    if "g2" not in a.shapes:
        not_run["g2"] = "not asked for (--shapes g2): the host route of 100 M lines takes tens of seconds per run and tens of GB"
    with tempfile.TemporaryDirectory() as folder:
        for shape in a.shapes:
            if shape == "g2" and available_bytes() < G2_HOST_BYTES:
                not_run["g2"] = f"not run: the host route needs about {G2_HOST_BYTES >> 30} GB, {available_bytes() >> 30} GB are available"
                continue
            path = os.path.join(folder, shape + ".lscc")
            results.append(probe(shape, path, a.reps))
            if a.kernel_stats:
                results[-1]["kernels"] = kernel_stats(path, results[-1])
            os.remove(path)
            print(json.dumps(results[-1]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:                             # (after every shape: a later one may run out of time)
                json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, host_threads=os.environ.get("OMP_NUM_THREADS"),
                               hbm_peak_tb_per_s=HBM_PEAK / 1e12, not_run=not_run, results=results), f, indent=1)
