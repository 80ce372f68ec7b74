"""Times the fused any-width MoCo step (MoCoTrainStep._body over csrc/ginx.hip) with f32 and with bf16 operands on the MI355X,
in one process and on one sampled batch stream:

  f32    GraphEncoder(encoder_dtype="f32"), MemoryMoCo(nce_dtype="f32")   -- ginx_gemm_kernel, v_mfma_f32_16x16x4_f32
  bf16   GraphEncoder(encoder_dtype="bf16"), MemoryMoCo(nce_dtype="bf16") -- ginx_gemm_bf16_kernel, v_mfma_f32_16x16x32_bf16

hidden 256, bsz 256, K 16384, rw_hops 256.  The batches are sampled and embedded once, outside the timed region, and cycled, so a
step is the training stream alone: both forwards, the head, the backward, clip + Adam + EMA + meters, the enqueue.  Per mode and
repetition: --warmup steps, then --steps steps between two device synchronisations (wall clock / steps).  The modes alternate,
--reps times; the spread of a mode is max - min over its repetitions.  Writes profiles/wide_bf16_probe.json and prints it.

    python tools/wide_bf16_probe.py [--steps 60] [--warmup 10] [--reps 3] [--modes f32,bf16]

Kernel times: run the same probe under `rocprofv3 --kernel-trace --stats -- python tools/wide_bf16_probe.py --reps 1 --no-json`
(a run of its own: no counters, no other tracing) and compare the summed time of ginx_gemm_kernel and ginx_gemm_bf16_kernel.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gcc_amd.contrast import MemoryMoCo  # noqa: E402
from gcc_amd.encoder import GraphEncoder  # noqa: E402
from gcc_amd.graph import DeviceGraph  # noqa: E402
from gcc_amd.graphgen import powerlaw_graph  # noqa: E402
from gcc_amd.posemb import DevicePosEmb  # noqa: E402
from gcc_amd.sampler import DeviceRWRSampler  # noqa: E402
from gcc_amd.train_step import MoCoTrainStep  # noqa: E402


def encoder(hidden, dtype):
    return GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=512, freq_embedding_size=16,
                        degree_embedding_size=16, output_dim=hidden, node_hidden_dim=hidden, edge_hidden_dim=hidden, num_layers=5,
                        num_step_set2set=6, num_layer_set2set=3, norm=True, gnn_model="gin", degree_input=True, encoder_dtype=dtype)


class Stream:
    """``n`` batches, sampled and embedded once, handed out in a cycle (the sampler interface of MoCoTrainStep)"""

    def __init__(self, B, hops, n, dev):
        rp, ci = powerlaw_graph(1_000_000, 10_000_000, seed=0)
        g = DeviceGraph(rp, ci, rw_hops=hops, restart_prob=0.8, device=dev, validate=False, trusted=True)
        s = DeviceRWRSampler(g, B, run_seed=0, num_buffers=2 * n)
        pe = DevicePosEmb(B, s.node_cap, 32, device=dev, seed=0, num_buffers=2 * n, max_views=2)
        self.batch_size, self.pairs = B, []
        for i in range(n):
            q, k = s.sample(i * B)
            pe(q)
            pe(k)
            self.pairs.append((q, k))
        s.check_status()
        pe.check_status(strict=True)
        torch.cuda.synchronize()
        self.keep = (g, s, pe)
        self.nodes = [int(q.node_off[B]) for q, _ in self.pairs]

    def sample(self, first_id, prof=None):
        return self.pairs[(first_id // self.batch_size) % len(self.pairs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", type=str, default="f32,bf16")
    ap.add_argument("--hidden-size", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--nce-k", type=int, default=16384)
    ap.add_argument("--rw-hops", type=int, default=256)
    ap.add_argument("--no-json", action="store_true", help="do not write profiles/wide_bf16_probe.json (profiler runs)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = Stream(a.batch_size, a.rw_hops, 8, dev)
    modes = a.modes.split(",")
    trainers, nstep = {}, {}
    for m in modes:
        torch.manual_seed(0)
        model, ema = encoder(a.hidden_size, m).to(dev), encoder(a.hidden_size, m).to(dev)
        ema.load_state_dict(model.state_dict())
        contrast = MemoryMoCo(a.hidden_size, None, a.nce_k, 0.07, use_softmax=True, nce_dtype=m).to(dev)
        trainers[m] = MoCoTrainStep(model, ema, contrast, stream, posemb=lambda g: g, prefetch=False)
        assert trainers[m].wide
        nstep[m] = 0
    ms = {m: [] for m in modes}
    losses = {}
    for _ in range(a.reps):
        for m in modes:
            tr = trainers[m]
            for _ in range(a.warmup):
                tr.step(nstep[m], 0.005)
                nstep[m] += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                out = tr.step(nstep[m], 0.005)
                nstep[m] += 1
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) * 1e3 / a.steps)
            losses[m] = float(out["loss"])
    res = dict(tool="wide_bf16_probe", hidden=a.hidden_size, batch_size=a.batch_size, nce_k=a.nce_k, rw_hops=a.rw_hops, steps=a.steps,
               warmup=a.warmup, reps=a.reps, nodes_per_view=stream.nodes, device=torch.cuda.get_device_name(0),
               ms_per_step={m: [round(v, 4) for v in ms[m]] for m in modes},
               median_ms={m: round(sorted(ms[m])[len(ms[m]) // 2], 4) for m in modes},
               spread_ms={m: round(max(ms[m]) - min(ms[m]), 4) for m in modes}, last_loss=losses)
    if "f32" in ms and "bf16" in ms:
        res["f32_over_bf16"] = round(res["median_ms"]["f32"] / res["median_ms"]["bf16"], 4)
    line = json.dumps(res)
    if not a.no_json:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "wide_bf16_probe.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
