"""Times one GAT MoCo step (train.py --model gat --moco) two ways on the MI355X, in one process and alternated step by step:

  hip    GraphEncoder(gnn_model="gat") on csrc/gat.hip (one forward launch, three backward launches per pass)
  torch  the same model with the encoder replaced by the plain-torch composition of tests/gat_reference.py, run in fp32
         on the device (index_add / index_reduce edge softmax, a Python loop over the T Set2Set steps and Lr LSTM layers)

Both steps: q forward + backward, k forward (model_ema, no grad), MemoryMoCo + NCESoftmaxLoss, clip_grad_norm, Adam, EMA.
Batches are sampled and embedded once (bsz 256, rw_hops 256, synthetic power-law graph) outside the timed region and
cycled.  GPU time by events: the whole step, and the encoder part (both forwards and the backward, which includes the
small head backward).  Median over --steps after --warmup.  Prints one JSON line.

    python tools/gat_probe.py [--steps 60] [--mode both|hip|torch]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gcc_amd.contrast import MemoryMoCo, NCESoftmaxLoss  # noqa: E402
from gcc_amd.encoder import GraphEncoder  # noqa: E402
from gcc_amd.graph import DeviceGraph  # noqa: E402
from gcc_amd.graphgen import powerlaw_graph  # noqa: E402
from gcc_amd.posemb import DevicePosEmb  # noqa: E402
from gcc_amd.sampler import DeviceRWRSampler  # noqa: E402
from gcc_amd.train_step import clip_grad_norm, flatten_parameters, moment_update  # noqa: E402
from tests.gat_reference import forward_of  # noqa: E402

KW = dict(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=512, freq_embedding_size=16,
          degree_embedding_size=16, output_dim=64, node_hidden_dim=64, edge_hidden_dim=64, num_layers=5, num_heads=4,
          num_step_set2set=6, num_layer_set2set=3, norm=True, gnn_model="gat", degree_input=True)


class TorchGat(torch.nn.Module):
    """the plain-torch composition: the restatement over the model's own fp32 parameters"""

    def __init__(self, enc):
        super().__init__()
        self.enc = enc

    def forward(self, view):
        g, host = view
        return forward_of(self.enc, dict(self.enc.named_parameters()), host)


def batches(B, hops, n, dev):
    rp, ci = powerlaw_graph(200_000, 2_000_000, 0)
    g = DeviceGraph(rp, ci, rw_hops=hops, device=dev)
    s = DeviceRWRSampler(g, batch_size=B, run_seed=3, num_buffers=2 * n)
    pe = DevicePosEmb(B, s.node_cap, 32, device=dev, seed=3, num_buffers=2 * n)
    out = []
    for i in range(n):
        q, k = s.sample(i)
        pe(q)
        pe(k)
        views = []
        for v in (q, k):
            nn_ = v.number_of_nodes()
            host = dict(node_off=v.node_off[: B + 1].long(), row_ptr=v.row_ptr[: nn_ + 1].long(),
                        col_idx=v.col_idx[: int(v.row_ptr[nn_])].long(), pos_undirected=v.pos_undirected[:nn_])
            views.append((v, host))
        out.append(views)
    s.check_status()
    pe.check_status(strict=True)
    torch.cuda.synchronize()
    return out


class Step:
    def __init__(self, kind, dev, K):
        torch.manual_seed(0)
        self.model, self.ema = GraphEncoder(**KW).to(dev), GraphEncoder(**KW).to(dev)
        flatten_parameters(self.model)
        flatten_parameters(self.ema)
        moment_update(self.model, self.ema, 0)
        self.ema.eval()
        self.kind = kind
        self.fq = TorchGat(self.model) if kind == "torch" else None
        self.fk = TorchGat(self.ema) if kind == "torch" else None
        self.contrast = MemoryMoCo(64, None, K, 0.07, use_softmax=True).to(dev)
        self.crit = NCESoftmaxLoss()
        self.opt = torch.optim.Adam(self.model.parameters(), lr=0.005, betas=(0.9, 0.999), weight_decay=1e-5)
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]

    def __call__(self, views):
        (q, hq), (k, hk) = views
        ev = self.ev
        ev[0].record()
        feat_q = self.fq((q, hq)) if self.fq else self.model(q)
        with torch.no_grad():
            feat_k = self.fk((k, hk)) if self.fk else self.ema(k)
        ev[1].record()
        out = self.contrast(feat_q, feat_k)
        loss = self.crit(out)
        self.opt.zero_grad()
        ev[2].record()
        loss.backward()
        ev[3].record()
        clip_grad_norm(list(self.model.parameters()), 1.0)
        self.opt.step()
        moment_update(self.model, self.ema, 0.999)
        ev[4].record()
        return loss

    def times(self):
        torch.cuda.synchronize()
        e = self.ev
        return e[0].elapsed_time(e[4]), e[0].elapsed_time(e[1]) + e[2].elapsed_time(e[3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--bsz", type=int, default=256)
    ap.add_argument("--nce-k", type=int, default=16384)
    ap.add_argument("--rw-hops", type=int, default=256)
    ap.add_argument("--mode", default="both", choices=["both", "hip", "torch"])
    a = ap.parse_args()
    dev = "cuda:0"
    data = batches(a.bsz, a.rw_hops, 4, dev)
    kinds = ["hip", "torch"] if a.mode == "both" else [a.mode]
    steps = {k: Step(k, dev, a.nce_k) for k in kinds}
    res = {k: dict(step=[], enc=[], loss=None) for k in kinds}
    for i in range(a.warmup + a.steps):
        for k in kinds:                                     # alternated: hip, torch, hip, torch, ...
            loss = steps[k](data[i % len(data)])
            t_step, t_enc = steps[k].times()
            if i >= a.warmup:
                res[k]["step"].append(t_step)
                res[k]["enc"].append(t_enc)
            res[k]["loss"] = float(loss)
    line = dict(probe="gat_moco_step", bsz=a.bsz, nce_k=a.nce_k, rw_hops=a.rw_hops, steps=a.steps, warmup=a.warmup,
                nodes_q=int(data[0][0][1]["node_off"][-1]), entries_q=int(data[0][0][1]["col_idx"].numel()))
    for k in kinds:
        line[k] = dict(step_ms_median=statistics.median(res[k]["step"]), encoder_fwd_bwd_ms_median=statistics.median(res[k]["enc"]),
                       last_loss=res[k]["loss"])
    if len(kinds) == 2:
        line["encoder_speedup_torch_over_hip"] = line["torch"]["encoder_fwd_bwd_ms_median"] / line["hip"]["encoder_fwd_bwd_ms_median"]
        line["step_speedup_torch_over_hip"] = line["torch"]["step_ms_median"] / line["hip"]["step_ms_median"]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
