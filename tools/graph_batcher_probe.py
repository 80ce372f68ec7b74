"""Times the two batchers of the whole-graph datasets on the MI355X, host (the NumPy loop of gcc_amd/datasets.py) against device
(gcc_pack_graphs), on two synthetic corpora of rings plus random chords:

  imdb-like   1,000 graphs of 12-30 nodes,   batch size 32
  rdt-b-like    600 graphs of 100-900 nodes, batch sizes 32 and 256

  (a) production   one epoch of ``dataset.batches(order)`` alone, ending in a device synchronise -> ms per batch
  (b) epoch        a fused fine-tuning epoch (LabeledProducer with prefetch + FinetuneTrainStep), wall clock including
                   production, after a warm-up epoch, ending in a device synchronise -> ms per step

Three repetitions, host and device alternated, in one process.  Both datasets get the same injected table of positional rows
(the eigensolver runs once per dataset whichever batcher is used and is not what differs).  Raw numbers go to --out.

    python tools/graph_batcher_probe.py [--out profiles/graph_batcher_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcc_amd.datasets import GraphClassificationDatasetLabeled  # noqa: E402
from gcc_amd.finetune import FinetuneTrainStep, LabeledProducer, clear_bn  # noqa: E402
from tools.finetune_probe import encoder  # noqa: E402


def ring_with_chords(n, rng):
    """simple symmetric CSR of a ring of n nodes plus n random chords"""
    a = np.concatenate([np.arange(n), rng.integers(0, n, n)])
    b = np.concatenate([(np.arange(n) + 1) % n, rng.integers(0, n, n)])
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    und = np.unique(lo * n + hi)
    src, dst = np.concatenate([und // n, und % n]), np.concatenate([und % n, und // n])
    order = np.lexsort((dst, src))
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(src, minlength=n))
    return rp, dst[order].astype(np.int64)


def corpus(kind, rng):
    count, lo, hi = (1000, 12, 31) if kind == "imdb-like" else (600, 100, 901)
    graphs = [ring_with_chords(int(n), rng) for n in rng.integers(lo, hi, count)]
    return graphs, rng.integers(0, 2, count)


def production_ms(ds, order, min_seconds=0.3):
    """ms per batch of batches(order) alone (at least three epochs and ``min_seconds``)"""
    batches, epochs = 0, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while epochs < 3 or time.perf_counter() - t0 < min_seconds:
        for _g, _y in ds.batches(order):
            batches += 1
        epochs += 1
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / batches


def epoch_ms(ds, step, prod, order, min_seconds=0.3):
    """ms per step of fused fine-tuning epochs, production included"""
    steps, epochs = 0, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while epochs < 2 or time.perf_counter() - t0 < min_seconds:
        for g, y in prod.batches(order):
            step.step(steps, g, y, 0.005)
            steps += 1
        epochs += 1
        torch.cuda.synchronize()
    ds.check_status()
    return (time.perf_counter() - t0) * 1e3 / steps


def summary(xs):
    return dict(runs=[round(x, 4) for x in xs], median=round(float(np.median(xs)), 4), spread=round(max(xs) - min(xs), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "graph_batcher_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    results = []
    for kind, sizes in (("imdb-like", (32,)), ("rdt-b-like", (32, 256))):
        graphs, labels = corpus(kind, rng)
        table = torch.randn(sum(len(rp) - 1 for rp, _ in graphs), 32, device=dev)
        for B in sizes:
            ds = {}
            for b in ("host", "device"):
                ds[b] = GraphClassificationDatasetLabeled(graphs=graphs, labels=labels, rw_hops=256, batch_size=B, device=dev,
                                                          batcher=b)
                ds[b]._pos = table
            torch.manual_seed(0)
            model, head = encoder(dev), nn.Linear(64, 2).to(dev)
            step = FinetuneTrainStep(model, head)
            clear_bn(model)
            prod = {b: LabeledProducer(ds[b], dev) for b in ds}
            order = rng.permutation(len(graphs))
            for b in ds:                                           # warm-up: one epoch of each measurement
                production_ms(ds[b], order, 0.0)
                epoch_ms(ds[b], step, prod[b], order, 0.0)
            prod_ms, ep_ms = {b: [] for b in ds}, {b: [] for b in ds}
            for _ in range(a.reps):                                # alternated: host, device, host, device, ...
                for b in ds:
                    prod_ms[b].append(production_ms(ds[b], order))
                for b in ds:
                    ep_ms[b].append(epoch_ms(ds[b], step, prod[b], order))
            row = dict(corpus=kind, graphs=len(graphs), bsz=B, batches_per_epoch=(len(graphs) + B - 1) // B,
                       production_ms_per_batch={b: summary(v) for b, v in prod_ms.items()},
                       epoch_ms_per_step={b: summary(v) for b, v in ep_ms.items()})
            for key in ("production_ms_per_batch", "epoch_ms_per_step"):
                h, d = row[key]["host"], row[key]["device"]
                row[key]["device_faster_beyond_spread"] = bool(min(h["runs"]) > max(d["runs"]) and
                                                               h["median"] - d["median"] > max(h["spread"], d["spread"]))
            print(json.dumps(row), flush=True)
            results.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
