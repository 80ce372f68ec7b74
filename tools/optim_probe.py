"""Times one MoCo pre-training step (bsz 256, K 16384, rw_hops 256, hidden 64) and one fine-tuning step (bsz 32) per
--optimizer (adam, sgd, adagrad) the two ways ``train.py --step-path`` selects on the MI355X:

  fused  MoCoTrainStep / FinetuneTrainStep(optimizer=...): flat buffers, clip + update (+ EMA + meters) in two launches; the MoCo step
         both launch by launch ("fused_eager") and as a replayed hipGraph ("fused_graph": what train.py runs)
  api    autograd through GraphEncoder.forward and the heads, torch's clip, torch.optim, moment_update

on the same prepared batches (sampled and embedded once, outside the timed region: the step is timed, not the data pipeline).
All variants live in one process and are timed in alternation, ``--rounds`` times (default 5); a timing is a host clock around
``--steps`` steps that ends in a device synchronise, after warm-up steps of its own.  The result -- every raw timing and the
medians -- is one JSON document (``--out``, default profiles/optim_probe.json) and is printed.  No ratio is asserted.

    python tools/optim_probe.py [--steps 50] [--rounds 5] [--out profiles/optim_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gcc_amd.contrast import MemoryMoCo, NCESoftmaxLoss  # noqa: E402
from gcc_amd.datasets import GraphClassificationDatasetLabeled  # noqa: E402
from gcc_amd.encoder import GraphEncoder  # noqa: E402
from gcc_amd.finetune import FinetuneTrainStep, clear_bn, cls_head_loss  # noqa: E402
from gcc_amd.graph import DeviceGraph  # noqa: E402
from gcc_amd.graphgen import powerlaw_graph  # noqa: E402
from gcc_amd.posemb import DevicePosEmb  # noqa: E402
from gcc_amd.sampler import DeviceRWRSampler  # noqa: E402
from gcc_amd.train_step import MoCoTrainStep, clip_grad_norm, flatten_parameters, moment_update  # noqa: E402

OPTIMIZERS = ("adam", "sgd", "adagrad")
LR, WD, MOMENTUM, LR_DECAY = 0.005, 1e-5, 0.9, 0.0          # train.py's defaults


def encoder(dev):
    return GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=512,
                        freq_embedding_size=16, degree_embedding_size=16, output_dim=64, node_hidden_dim=64,
                        edge_hidden_dim=64, num_layers=5, num_step_set2set=6, num_layer_set2set=3, norm=True,
                        gnn_model="gin", degree_input=True).to(dev)


def torch_optimizer(name, params):
    if name == "adam":
        return torch.optim.Adam(params, lr=LR, betas=(0.9, 0.999), weight_decay=WD)
    if name == "sgd":
        return torch.optim.SGD(params, lr=LR, momentum=MOMENTUM, weight_decay=WD)
    return torch.optim.Adagrad(params, lr=LR, lr_decay=LR_DECAY, weight_decay=WD)


class Prepared:
    """a sampler that hands out batches made before the timed region, round robin"""

    def __init__(self, pairs, B):
        self.pairs, self.batch_size = pairs, B

    def sample(self, first_id, prof=None):
        return self.pairs[(first_id // self.batch_size) % len(self.pairs)]


def moco_variants(dev, B, K, rw_hops):
    rp, ci = powerlaw_graph(200_000, 2_000_000, 0)
    graph = DeviceGraph(rp, ci, rw_hops=rw_hops, device=dev)
    smp = DeviceRWRSampler(graph, B, run_seed=0, num_buffers=4)
    pe = DevicePosEmb(B, smp.node_cap, 32, device=dev, seed=0, num_buffers=8)
    pairs = []
    for i in range(4):
        q, k = smp.sample(i * B)
        pe(q)
        pe(k)
        pairs.append((q, k))
    smp.check_status()
    pe.check_status()
    torch.cuda.synchronize()
    out = {}
    for name in OPTIMIZERS:
        for graph_replay in (False, True):
            torch.manual_seed(0)
            model, ema = encoder(dev), encoder(dev)
            ema.load_state_dict(model.state_dict())
            contrast = MemoryMoCo(64, None, K, 0.07, use_softmax=True).to(dev)
            tr = MoCoTrainStep(model, ema, contrast, Prepared(pairs, B), posemb=lambda g, prof=None: g, prefetch=False,
                               graph=graph_replay, optimizer=name, momentum=MOMENTUM, lr_decay=LR_DECAY, weight_decay=WD)
            tr.relaxed_streams = True
            out[(name, "fused_graph" if graph_replay else "fused_eager")] = lambda i, tr=tr: tr.step(i, LR)
        torch.manual_seed(0)
        model, ema = encoder(dev), encoder(dev)
        flatten_parameters(model)
        flatten_parameters(ema)
        moment_update(model, ema, 0)
        contrast = MemoryMoCo(64, None, K, 0.07, use_softmax=True).to(dev)
        opt = torch_optimizer(name, model.parameters())
        crit = NCESoftmaxLoss()
        model.train()
        ema.eval()
        for mod in ema.modules():
            if isinstance(mod, nn.BatchNorm1d):
                mod.train()

        def api(i, model=model, ema=ema, contrast=contrast, opt=opt, crit=crit):          # train.py's API branch
            q, k = pairs[i % len(pairs)]
            feat_q = model(q)
            with torch.no_grad():
                feat_k = ema(k)
            logits = contrast(feat_q, feat_k)
            opt.zero_grad()
            crit(logits).backward()
            clip_grad_norm(list(model.parameters()), 1.0)
            for grp in opt.param_groups:
                grp["lr"] = LR
            opt.step()
            moment_update(model, ema, 0.999)

        out[(name, "api")] = api
    return out


def finetune_variants(dev, B):
    rng = np.random.default_rng(0)
    graphs = [powerlaw_graph(20 + int(rng.integers(0, 60)), 80 + int(rng.integers(0, 300)), 1000 + i) for i in range(512)]
    ds = GraphClassificationDatasetLabeled(graphs=graphs, labels=rng.integers(0, 2, len(graphs)), rw_hops=256, batch_size=B,
                                           device=dev, num_buffers=8)
    order = np.arange(len(ds))
    batches = []
    for i in range(4):
        g, y = ds.make_batch(order[i * B:(i + 1) * B])
        for a in ("node_off", "edge_off", "row_ptr", "col_idx", "graph_id", "parent_nid", "pos_undirected"):
            if getattr(g, a, None) is not None:            # (keep each batch's ring-slot buffers: copy what later calls reuse)
                setattr(g, a, getattr(g, a).clone())
        batches.append((g, y.clone()))
    out = {}
    for name in OPTIMIZERS:
        torch.manual_seed(0)
        model, head = encoder(dev), nn.Linear(64, 2).to(dev)
        step = FinetuneTrainStep(model, head, optimizer=name, momentum=MOMENTUM, lr_decay=LR_DECAY, weight_decay=WD)
        clear_bn(model)
        out[(name, "fused_eager")] = lambda i, step=step: step.step(i, *batches[i % len(batches)], LR)
        model2, head2 = encoder(dev), nn.Linear(64, 2).to(dev)
        opt = torch_optimizer(name, model2.parameters())
        hopt = torch.optim.Adam(head2.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=WD)

        def api(i, model2=model2, head2=head2, opt=opt, hopt=hopt):                      # finetune_main's API branch
            g, y = batches[i % len(batches)]
            model2.train()
            loss = cls_head_loss(model2(g), head2, y)[0]
            opt.zero_grad()
            hopt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_value_(model2.parameters(), 1)
            torch.nn.utils.clip_grad_value_(head2.parameters(), 1)
            opt.step()
            hopt.step()

        out[(name, "api")] = api
    return out


def timed(fn, first, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(first, first + steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def measure(variants, steps, rounds, warmup=8):
    done = {key: 0 for key in variants}
    for key, fn in variants.items():                       # first launches load code objects; the replayed step captures here
        timed(fn, 0, warmup)
        done[key] = warmup
    raw = {key: [] for key in variants}
    for _ in range(rounds):
        for key, fn in variants.items():                   # alternated: every round visits every variant once
            raw[key].append(timed(fn, done[key], steps))
            done[key] += steps
    return raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "optim_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "optim_probe measures on the GPU: there is nothing to time without one"
    dev = torch.device("cuda:0")
    doc = dict(device=torch.cuda.get_device_name(0), steps_per_timing=a.steps, rounds=a.rounds, unit="ms per step",
               hyperparameters=dict(lr=LR, weight_decay=WD, momentum=MOMENTUM, lr_decay=LR_DECAY), cases=[])
    for case, variants in (("moco_step bsz 256 K 16384 rw_hops 256 hidden 64", moco_variants(dev, 256, 16384, 256)),
                           ("finetune_step bsz 32 graph classification", finetune_variants(dev, 32))):
        raw = measure(variants, a.steps, a.rounds)
        for (name, path), ts in raw.items():
            row = dict(case=case, optimizer=name, path=path, median_ms=round(statistics.median(ts), 4), raw_ms=[round(t, 4) for t in ts])
            doc["cases"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
