"""generate.py's embedding loop (generate.py:33-53) with a WIDE GIN encoder (hidden 256, 4 GIN layers): the eval chain --
two passes of gcc_ginx_forward, one launch per operator, and a torch mean -- against GraphEncoder.resident_eval, one
gcc_ginw_embed call per batch (bf16 layers resident in LDS, f32 readout).  One pre-sampled stream of batches per rw_hops
setting (sampler and positional embedding are the same for both paths and stay outside the clock); the two paths are timed
alternately, three repetitions each after a warm-up of every shape, device events around a window of calls long enough to
be a fraction of a second.  Per path and setting: GPU time per call (device events) and wall time per call (host clock
around the same window, synchronised), raw numbers, medians and spreads -> profiles/wide_eval_probe.json.

    python tools/wide_eval_probe.py [--out profiles/wide_eval_probe.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/wide_eval_probe.py --only resident --windows 1 --out DIR/probe.json

``--only`` limits the run to one path (the kernel-trace runs: one path per trace, so that the kernel sums are that path's).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcc_amd.encoder import GraphEncoder
from gcc_amd.graph import DeviceGraph
from gcc_amd.graphgen import powerlaw_graph
from gcc_amd.posemb import DevicePosEmb
from gcc_amd.sampler import DeviceRWRSampler

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=10000)
ap.add_argument("--edges", type=int, default=100000)
ap.add_argument("--batch-size", type=int, default=256)
ap.add_argument("--rw-hops", type=int, nargs="+", default=[64, 256])
ap.add_argument("--batches", type=int, default=4, help="pre-sampled batches per setting (the stream a window walks)")
ap.add_argument("--rounds", type=int, default=16, help="times a window walks the stream: calls per window = batches x rounds")
ap.add_argument("--windows", type=int, default=3, help="timed repetitions per path and setting")
ap.add_argument("--only", choices=["chain", "resident"], default=None)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wide_eval_probe.json"))
a = ap.parse_args()
dev = torch.device("cuda:0")
B = a.batch_size
rp, ci = powerlaw_graph(a.nodes, a.edges, seed=1)
torch.manual_seed(0)
model = GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=512, freq_embedding_size=16,
                     degree_embedding_size=16, output_dim=256, node_hidden_dim=256, edge_hidden_dim=256, num_layers=5,
                     num_step_set2set=6, num_layer_set2set=3, norm=True, gnn_model="gin", degree_input=True).to(dev)
model.eval()


def run_path(path, stream):
    model.resident_eval = path == "resident"
    out = None
    for q, k in stream:
        out = model.embed_views(q, k)
    return out


def window(path, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.rounds):
        run_path(path, stream)
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    calls = a.rounds * len(stream)
    return e0.elapsed_time(e1) * 1e3 / calls, wall * 1e6 / calls           # us per call: device events, host clock


paths = [a.only] if a.only else ["chain", "resident"]
report = dict(config=dict(hidden=256, gin_layers=4, batch_size=B, views=2, nodes=a.nodes, edges=len(ci), batches=a.batches,
                          calls_per_window=a.batches * a.rounds, windows=a.windows, device=torch.cuda.get_device_name(0)), settings=[])
for hops in a.rw_hops:
    graph = DeviceGraph(rp, ci, rw_hops=hops, device=dev)
    smp = DeviceRWRSampler(graph, B, run_seed=0, num_buffers=a.batches)
    pe = DevicePosEmb(B, smp.node_cap, 32, device=dev, seed=0, max_views=2, num_buffers=a.batches)
    stream = []
    for i in range(a.batches):
        q, k = smp.sample(i * B)
        pe.multi([q, k])
        for v in (q, k):
            v.edge_multiplicity = 2                                          # generate.py on an edge list
        stream.append((q, k))
    smp.check_status()
    sizes = torch.cat([torch.diff(v.node_off[: B + 1]) for pair in stream for v in pair]).cpu()
    for p in paths:                                                          # warm-up of every shape: allocations, the fold, the LDS opt-in
        for _ in range(2):
            run_path(p, stream)
    torch.cuda.synchronize()
    raw = {p: dict(gpu_us=[], wall_us=[]) for p in paths}
    for _ in range(a.windows):                                               # alternately
        for p in paths:
            g, w = window(p, stream)
            raw[p]["gpu_us"].append(g)
            raw[p]["wall_us"].append(w)
    if "resident" in paths:
        model.resident_engine().check_status()
    entry = dict(rw_hops=hops, subgraph_nodes=dict(median=int(sizes.median()), max=int(sizes.max()),
                                                   over_128=int((sizes > 128).sum()), subgraphs=int(sizes.numel())), paths={})
    for p in paths:
        entry["paths"][p] = {k: dict(raw=v, median=statistics.median(v), spread=max(v) - min(v)) for k, v in raw[p].items()}
    if len(paths) == 2:
        with torch.no_grad():
            fc, fr = run_path("chain", stream[:1]), run_path("resident", stream[:1])
        entry["max_abs_difference_of_unit_norm_embeddings"] = float((fc - fr).abs().max())
        c, r = entry["paths"]["chain"]["gpu_us"], entry["paths"]["resident"]["gpu_us"]
        entry["gpu_ratio_chain_over_resident"] = c["median"] / r["median"]
        entry["wall_ratio_chain_over_resident"] = entry["paths"]["chain"]["wall_us"]["median"] / entry["paths"]["resident"]["wall_us"]["median"]
        entry["resident_wins_by_more_than_the_larger_spread"] = bool(c["median"] - r["median"] > max(c["spread"], r["spread"]))
    report["settings"].append(entry)
    print(json.dumps(entry))
    del smp, pe, graph, stream
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
    f.write("\n")
print("wrote", a.out)
