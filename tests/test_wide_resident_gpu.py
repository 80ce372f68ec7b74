"""GraphEncoder.resident_eval / gcc_ginw_embed on the MI355X: sampled batches (DeviceRWRSampler + DevicePosEmb) through
``embed_views`` as one LDS-resident bf16 call, against tests/wide_resident_reference.py and against the f32 eval chain
of the same weights.  The emulator tier (shape edges, refusals, the fold cache, generate.py) is
tests/test_wide_resident_emu.py."""
import numpy as np
import pytest
import torch

from tests import wide_resident_reference as R

pytestmark = pytest.mark.gpu

B = 8
HUB_DEGREE = 600


def random_graph(n=2000, avg_deg=8, hub_degree=0, seed=0):
    """simple symmetric graph on n nodes; with ``hub_degree`` node 0 is adjacent to that many others"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, n * avg_deg // 2)
    dst = rng.integers(0, n, n * avg_deg // 2)
    ring = np.arange(n)
    src, dst = np.concatenate([src, ring]), np.concatenate([dst, (ring + 1) % n])          # connected
    if hub_degree:
        nb = rng.choice(np.arange(1, n), size=hub_degree, replace=False)
        keep = (src != 0) & (dst != 0)
        src, dst = np.concatenate([src[keep], np.zeros(hub_degree, dtype=np.int64)]), np.concatenate([dst[keep], nb])
    keep = src != dst
    a, b = np.concatenate([src[keep], dst[keep]]), np.concatenate([dst[keep], src[keep]])
    pairs = np.unique(a * n + b)
    a, b = pairs // n, pairs % n
    row_ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(a, minlength=n), out=row_ptr[1:])
    return row_ptr, b.astype(np.int32)


def models(seed):
    """the resident model and an encoder_dtype="f32" model with the same weights on the chain"""
    from gcc_amd.encoder import GraphEncoder

    kw = dict(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=512, freq_embedding_size=16,
              degree_embedding_size=16, output_dim=256, node_hidden_dim=256, edge_hidden_dim=256, num_layers=3, num_step_set2set=6,
              num_layer_set2set=3, norm=True, gnn_model="gin", degree_input=True)
    torch.manual_seed(seed)
    enc = GraphEncoder(**kw)
    R.randomize_running_stats(enc, seed + 1)
    enc = enc.cuda().eval()
    chain = GraphEncoder(encoder_dtype="f32", **kw).cuda().eval()
    chain.load_state_dict(enc.state_dict())
    enc.resident_eval = True
    assert chain.resident_eval is False
    return enc, chain


def sampled_views(row_ptr, col_idx, rw_hops, seeds=None, mult=1):
    from gcc_amd.graph import DeviceGraph
    from gcc_amd.posemb import DevicePosEmb
    from gcc_amd.sampler import DeviceRWRSampler

    g = DeviceGraph(row_ptr, col_idx, rw_hops=rw_hops, device="cuda:0")
    smp = DeviceRWRSampler(g, batch_size=B, run_seed=5)
    q, k = smp.sample(0, seeds=None if seeds is None else torch.tensor(seeds, dtype=torch.int32, device="cuda:0"))
    smp.check_status()
    pe = DevicePosEmb(B, smp.node_cap, 32, device="cuda:0", seed=5, max_views=2)
    pe.multi([q, k])
    assert pe.check_status() == 0
    for v in (q, k):
        v.edge_multiplicity = mult
    return q, k


def check(enc, chain, q, k, mult, label):
    got = enc.embed_views(q, k)
    torch.cuda.synchronize()
    assert enc.resident_engine().check_status() == 0
    assert tuple(got.shape) == (B, 256) and bool(torch.isfinite(got).all())
    R.check_bars(got.cpu().numpy(), enc, [q, k], mult, label=label)
    want = chain.embed_views(q, k)          # two passes of the one-launch-per-operator chain and a torch mean, f32
    e_chain = R.graph_errors(got.cpu().numpy(), want.cpu().numpy())
    print(f"{label} per-graph error vs the f32 chain:  " + " ".join(f"{e:.1e}" for e in e_chain))
    assert (e_chain < R.BAR_TRUTH).all(), e_chain       # the chain is within 1e-3 of float64: the truth's bar applies


def test_resident_embedding_on_sampled_batches():
    enc, chain = models(0)
    row_ptr, col_idx = random_graph()
    q, k = sampled_views(row_ptr, col_idx, rw_hops=64, mult=2)       # multiplicity 2, as generate.py's edge lists have it
    sizes = torch.diff(q.node_off).cpu()
    assert int(sizes.min()) >= 1 and int(sizes.max()) <= 128
    check(enc, chain, q, k, 2, "rw_hops 64")


def test_resident_embedding_with_a_subgraph_over_128_nodes():
    enc, chain = models(1)
    row_ptr, col_idx = random_graph(hub_degree=HUB_DEGREE)
    assert int(np.diff(row_ptr)[0]) == HUB_DEGREE
    seeds = [0, 0, 0, 0, 17, 230, 1999, 0]                           # ego-nets of the hub, and a few ordinary ones
    q, k = sampled_views(row_ptr, col_idx, rw_hops=256, seeds=seeds)
    sizes = torch.cat([torch.diff(q.node_off), torch.diff(k.node_off)]).cpu()
    print("subgraph sizes:", sizes.tolist())
    assert int(sizes.max()) > 128 and int(sizes.min()) <= 128        # both kernels run
    check(enc, chain, q, k, 1, "rw_hops 256, hub seed")
