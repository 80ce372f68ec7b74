"""Times one fine-tuning step (train.py --finetune) two ways on the MI355X:

  fused  gcc_amd.finetune.FinetuneTrainStep: GIN forward / gcc_cls_head_train / GIN backward / two gcc_adam_clipvalue_step
  api    the composition the reference runs: GraphEncoder.forward through autograd + nn.Linear + nn.CrossEntropyLoss +
         clip_grad_value_ + two torch.optim.Adam

on the same prepared batches (sampled and embedded once, outside the timed region), at batch sizes 32 and 256, for a synthetic
labelled graph (node classification) and a synthetic set of small graphs (graph classification); plus the held-out eval
(gcc_amd.finetune.evaluate) of a fold.  Prints one JSON line per case.

    python tools/finetune_probe.py [--steps 50]
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

from gcc_amd.datasets import GraphClassificationDatasetLabeled, NodeClassificationDatasetLabeled  # noqa: E402
from gcc_amd.encoder import GraphEncoder  # noqa: E402
from gcc_amd.finetune import FinetuneTrainStep, clear_bn, cls_head_loss, evaluate  # noqa: E402
from gcc_amd.graphgen import powerlaw_graph  # noqa: E402


def encoder(dev):
    return GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=512,
                        freq_embedding_size=16, degree_embedding_size=16, output_dim=64, node_hidden_dim=64,
                        edge_hidden_dim=64, num_layers=5, num_step_set2set=6, num_layer_set2set=3, norm=True,
                        gnn_model="gin", degree_input=True).to(dev)


def timed(fn, batches, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i, *batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def run_case(kind, ds, C, B, steps, dev):
    order = np.arange(len(ds))
    batches = [ds.make_batch(order[i * B:(i + 1) * B]) for i in range(4)]
    batches = [(g, y.clone()) for g, y in batches]
    for g, _ in batches:                                   # (keep each batch's ring-slot buffers: copy what later calls reuse)
        for a in ("node_off", "edge_off", "row_ptr", "col_idx", "graph_id", "parent_nid", "pos_undirected"):
            if getattr(g, a, None) is not None:
                setattr(g, a, getattr(g, a).clone())
    torch.manual_seed(0)
    model, head = encoder(dev), nn.Linear(64, C).to(dev)
    step = FinetuneTrainStep(model, head)
    clear_bn(model)
    fused = lambda i, g, y: step.step(i, g, y, 0.005)                       # noqa: E731
    timed(fused, batches, 5)
    ms_fused = timed(fused, batches, steps)

    model2, head2 = encoder(dev), nn.Linear(64, C).to(dev)
    opt = torch.optim.Adam(model2.parameters(), lr=0.005, betas=(0.9, 0.999), weight_decay=1e-5)
    hopt = torch.optim.Adam(head2.parameters(), lr=0.005, betas=(0.9, 0.999), weight_decay=1e-5)
    crit = nn.CrossEntropyLoss()
    model2.train()

    def api(i, g, y):
        feat = model2(g)
        v = y >= 0
        loss = crit(head2(feat)[v], y[v].long())
        opt.zero_grad()
        hopt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_value_(model2.parameters(), 1)
        torch.nn.utils.clip_grad_value_(head2.parameters(), 1)
        opt.step()
        hopt.step()

    timed(api, batches, 5)
    ms_api = timed(api, batches, steps)

    model2.train()
    head_api = lambda i, g, y: cls_head_loss(model2(g), head2, y)[0].backward()    # noqa: E731  (the HIP head in autograd)
    timed(head_api, batches, 3)

    n_eval = min(len(ds), max(B * 4, len(ds) // 10))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, f1 = evaluate(model, head, ds, order[:n_eval])
    eval_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(kind=kind, bsz=B, classes=C, fused_ms_per_step=round(ms_fused, 3), api_ms_per_step=round(ms_api, 3),
                          eval_items=int(n_eval), eval_ms=round(eval_ms, 2), eval_loss=round(loss, 4), eval_f1=round(f1, 4))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--bsz", type=str, default="32,256")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rp, ci = powerlaw_graph(20000, 200000, 0)
    labels = rng.integers(0, 4, len(rp) - 1)
    graphs = [powerlaw_graph(20 + int(rng.integers(0, 60)), 80 + int(rng.integers(0, 300)), 1000 + i) for i in range(2000)]
    glabels = rng.integers(0, 2, len(graphs))
    for B in (int(x) for x in a.bsz.split(",")):
        node = NodeClassificationDatasetLabeled(graph=(rp, ci), labels=labels, rw_hops=256, batch_size=B, device=dev,
                                                num_buffers=8)
        run_case("node", node, 4, B, a.steps, dev)
        grp = GraphClassificationDatasetLabeled(graphs=graphs, labels=glabels, rw_hops=256, batch_size=B, device=dev,
                                                num_buffers=8)
        run_case("graph", grp, 2, B, a.steps, dev)


if __name__ == "__main__":
    main()
