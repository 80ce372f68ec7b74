"""The device reader of TU dataset text (gcc_text_ints_sep, gcc_tu_corpus; gcc_amd.tu_ingest) against the host route, each from
the folder's path to a ready ``DeviceGraphCorpus``, on one MI355X -> profiles/tu_ingest_probe.json.

    python tools/tu_ingest_probe.py [--reps 5] [--shapes collab hub] [--out profiles/tu_ingest_probe.json]

Per shape three seeded files are written to a temporary folder (``ingest.write_tudataset`` layout, ``u, v`` lines) and read once
(page cache).  After one warm-up of each route the two routes ALTERNATE in this process, ``reps`` times; every figure is the median,
wall clock, milliseconds:
  host    read_ms        ``ingest.read_tudataset(folder, name)``
          corpus_ms      ``DeviceGraphCorpus(graphs, 32, labels=...)``: the per-graph loop and the upload
          total_ms       both
  device  read_ms        ``TUIngestEngine.read_tudataset(folder, name)``
          corpus_ms      ``DeviceGraphCorpus.from_device(...)``
          total_ms       both, as a user runs them
          upload_ms, count_ms, parse_ms, build_ms, host_reads_ms   a second set of ``reps`` runs with a device synchronisation after
                         every stage, so that the stages can be told apart: the three file reads with their chunked copies; the
                         three count-only tokenizer calls; the three parsing calls; gcc_tu_corpus; the rest (the two host reads)
  host_over_device       host total_ms over device total_ms: above 1 the device wins, below 1 it loses.
  upload_share           upload_ms over the synchronised device read: the share of reading the files and copying them.
Shapes: ``collab`` about 5,000 graphs, 376 k nodes and 4.1 M lines (COLLAB-sized); ``hub`` 2,000 stars whose hub rows exceed
GCC_GRAPH_BUILD_LDS_ROW (the third sort class); ``small`` 1,000 graphs of about 20 nodes (IMDB-sized: where the fixed costs show).
Nothing here is asserted; losses stay in the JSON."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcc_amd import _cabi, ingest  # noqa: E402
from gcc_amd.datasets import DeviceGraphCorpus  # noqa: E402
from gcc_amd.text_ingest import TextIngestEngine  # noqa: E402
from gcc_amd.tu_ingest import TUIngestEngine  # noqa: E402

NAME, BATCH = "PROBE", 32


def lines_of(shape, seed=0):
    """-> (pairs int64 [m, 2] 1-based with both directions, indicator, labels)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    if shape == "hub":
        graphs, leaves = 2000, _cabi.GRAPH_BUILD_LDS_ROW + 100
        first = np.arange(graphs, dtype=np.int64) * (leaves + 1) + 1
        hub = np.repeat(first, leaves)
        leaf = hub + np.tile(np.arange(1, leaves + 1, dtype=np.int64), graphs)
        sizes = np.full(graphs, leaves + 1, dtype=np.int64)
        pairs = np.concatenate([np.stack([hub, leaf], 1), np.stack([leaf, hub], 1)])
    else:
        graphs, lo, hi, per = (5000, 40, 111, 6) if shape == "collab" else (1000, 10, 31, 3)
        sizes = rng.integers(lo, hi, size=graphs)
        first = np.concatenate([[0], np.cumsum(sizes)])
        parts = []
        for g in range(graphs):
            n = int(sizes[g])
            e = rng.integers(0, n, size=(per * n, 2))
            e = e[e[:, 0] != e[:, 1]]
            key = np.unique(np.minimum(e[:, 0], e[:, 1]) * n + np.maximum(e[:, 0], e[:, 1]))
            a, b = key // n + first[g] + 1, key % n + first[g] + 1
            parts += [np.stack([a, b], 1), np.stack([b, a], 1)]
        pairs = np.concatenate(parts)
    pairs = pairs[rng.permutation(len(pairs))]
    return pairs, np.repeat(np.arange(1, graphs + 1, dtype=np.int64), sizes), rng.integers(0, 3, size=graphs)


def write_files(folder, pairs, indicator, labels):
    base = os.path.join(folder, NAME + "_")
    with open(base + "A.txt", "wb") as f:
        for at in range(0, len(pairs), 1 << 20):
            f.write(b"".join(b"%d, %d\n" % (u, v) for u, v in pairs[at:at + (1 << 20)].tolist()))
    for kind, values in (("graph_indicator", indicator), ("graph_labels", labels)):
        with open(base + kind + ".txt", "wb") as f:
            f.write(b"".join(b"%d\n" % x for x in values.tolist()))
    total = 0
    for kind in ("A", "graph_indicator", "graph_labels"):
        with open(base + kind + ".txt", "rb") as f:                 # (page cache)
            while True:
                chunk = f.read(1 << 24)
                if not chunk:
                    break
                total += len(chunk)
    return total


class Clock:
    def __init__(self):
        self.ms = dict(upload=0.0, count=0.0, parse=0.0, build=0.0)

    def timed(self, key, fn, *a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a, **k)
        torch.cuda.synchronize()
        self.ms[key] += (time.perf_counter() - t0) * 1e3
        return out


class StagedText(TextIngestEngine):
    def __init__(self, clock, *a, **k):
        super().__init__(*a, **k)
        self.clock = clock

    def upload(self, *a, **k):
        return self.clock.timed("upload", super().upload, *a, **k)

    def ints_sep_into(self, text, nbytes, first_byte, max_tokens, *a, **k):
        return self.clock.timed("count" if max_tokens == 0 else "parse", super().ints_sep_into, text, nbytes, first_byte, max_tokens, *a, **k)


class Staged(TUIngestEngine):
    """the engine with a synchronisation and a clock after every stage of read_tudataset"""

    def __init__(self, device):
        self.clock = Clock()
        super().__init__(device=device)
        self.text = StagedText(self.clock, self.lib, self.ptr, device)

    def corpus_into(self, *a, **k):
        return self.clock.timed("build", super().corpus_into, *a, **k)


def probe(shape, folder, reps):
    pairs, indicator, labels = lines_of(shape)
    nbytes = write_files(folder, pairs, indicator, labels)
    out = dict(shape=shape, graphs=int(len(labels)), nodes=int(len(indicator)), lines=int(len(pairs)), file_bytes=nbytes)
    del pairs, indicator, labels
    engine = TUIngestEngine(device="cuda:0")

    def host_route():
        t0 = time.perf_counter()
        d = ingest.read_tudataset(folder, NAME)
        t1 = time.perf_counter()
        c = DeviceGraphCorpus(d["graphs"], BATCH, labels=d["graph_labels"], device="cuda:0")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return dict(read_ms=(t1 - t0) * 1e3, corpus_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3), c

    def device_route(eng=engine):
        t0 = time.perf_counter()
        d = eng.read_tudataset(folder, NAME)
        t1 = time.perf_counter()
        c = DeviceGraphCorpus.from_device(d["corpus"], BATCH, device="cuda:0")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return dict(read_ms=(t1 - t0) * 1e3, corpus_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3), c

    _, hc = host_route()                                            # (warm-up of each route; also the two results compared)
    _, dc = device_route()
    out["same_corpus"] = bool(all(torch.equal(getattr(hc, k), getattr(dc, k)) for k in ("node_first", "row_ptr", "col_idx", "seed_local", "labels"))
                              and np.array_equal(hc.sizes, dc.sizes) and np.array_equal(hc.entries, dc.entries))
    out["longest_row"] = int(torch.diff(dc.row_ptr).max())
    del hc, dc
    host, device = [], []
    for _ in range(reps):
        host.append(host_route()[0])
        device.append(device_route()[0])
    staged = []
    for _ in range(reps):
        eng = Staged("cuda:0")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.read_tudataset(folder, NAME)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        ms = eng.clock.ms
        staged.append(dict(upload_ms=ms["upload"], count_ms=ms["count"], parse_ms=ms["parse"], build_ms=ms["build"],
                           host_reads_ms=total - sum(ms.values()), read_synchronised_ms=total))

    def med(rows):
        return {k: statistics.median(r[k] for r in rows) for k in rows[0]}

    out["host"], out["device"] = med(host), {**med(device), **med(staged)}
    out["host_over_device"] = out["host"]["total_ms"] / out["device"]["total_ms"]
    out["upload_share"] = out["device"]["upload_ms"] / out["device"]["read_synchronised_ms"]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["collab", "hub", "small"], choices=["collab", "hub", "small"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tu_ingest_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tu_ingest_probe.py measures on the GPU: none found")
    results = []
    for shape in a.shapes:
        with tempfile.TemporaryDirectory() as folder:
            results.append(probe(shape, folder, a.reps))
        print(json.dumps(results[-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                                 # (after every shape: a later one may run out of time)
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, host_threads=os.environ.get("OMP_NUM_THREADS"), batch_size=BATCH,
                           results=results), f, indent=1)
