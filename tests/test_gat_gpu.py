"""The GAT backbone (csrc/gat.hip) on a real MI355X: a sampled bsz-256, rw_hops-256 batch at the defaults against the
float64 restatement (with torch fp32's error on the same inputs beside it), bit-identical gradients across two backward
calls, and train.py --model gat (MoCo, E2E, --finetune) plus generate.py end to end."""
import io
import os
import re
import subprocess
import sys
import types
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from tests.gat_check import gat_encoder, kernel_grads, reference, symmetric_batch, worst_rel
from tests.gat_reference import forward_of, params_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sampled_batch(B=256, hops=256, both=False):
    from gcc_amd.graph import DeviceGraph
    from gcc_amd.graphgen import powerlaw_graph
    from gcc_amd.posemb import DevicePosEmb
    from gcc_amd.sampler import DeviceRWRSampler

    rp, ci = powerlaw_graph(200000, 2000000, 0)
    g = DeviceGraph(rp, ci, rw_hops=hops, device="cuda:0")
    s = DeviceRWRSampler(g, batch_size=B, run_seed=3)
    q, k = s.sample(0)
    s.check_status()
    pe = DevicePosEmb(B, s.node_cap, 32, device="cuda:0", seed=3)
    pe(q)
    pe(k)
    pe.check_status(strict=True)
    torch.cuda.synchronize()

    def host(v):
        n = v.number_of_nodes()
        return dict(node_off=v.node_off[: B + 1].cpu().long(), row_ptr=v.row_ptr[: n + 1].cpu().long(),
                    col_idx=v.col_idx[: int(v.row_ptr[n])].cpu().long(), pos_undirected=v.pos_undirected[:n].cpu())

    return (q, host(q), k, host(k)) if both else (q, host(q))


def _seed_kw(v):
    sl = getattr(v, "seed_local", None)
    return {} if sl is None else dict(seed_local=sl[: v.batch_size].cpu().long())


def test_sampled_batch_against_float64_and_bit_identical():
    from gcc_amd.encoder import GatEngine

    q, host = _sampled_batch()
    kw = _seed_kw(q)
    enc = gat_encoder().cuda()
    dout = torch.randn(q.batch_size, 64, generator=torch.Generator().manual_seed(1)).cuda()
    eng = GatEngine()
    out, grads, _ = kernel_grads(enc, eng, q, dout)
    _, grads2, _ = kernel_grads(enc, eng, q, dout)
    torch.cuda.synchronize()
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k                  # no float atomics: bit-identical
    P = params_of(enc)
    ref = forward_of(enc, P, host, **kw)
    (ref * dout.cpu().double()).sum().backward()
    ref_grads = {k: v.grad for k, v in P.items()}
    # torch fp32 composition on the device, same inputs: the figure the kernels' error is weighed against
    P32 = {k: v.detach().cuda().float().requires_grad_(True) for k, v in enc.named_parameters()}
    dev_batch = {k: v.cuda() for k, v in host.items()}
    o32 = forward_of(enc, P32, dev_batch, **{k: v.cuda() for k, v in kw.items()})
    (o32 * dout).sum().backward()
    g32 = {k: v.grad for k, v in P32.items()}
    out_err = float((out.double().cpu() - ref.detach()).abs().max())
    worst, name = worst_rel(grads, ref_grads)
    worst32, name32 = worst_rel(g32, ref_grads)
    print(f"GAT sampled bsz 256: {int(host['node_off'][-1])} nodes, {len(host['col_idx'])} entries; out err {out_err:.2e}; "
          f"worst gradient entry / tensor max-abs vs float64: kernels {worst:.2e} ({name}), torch fp32 {worst32:.2e} ({name32})")
    assert out_err < 1e-4
    assert worst < max(1e-3, 2 * worst32), (worst, name, worst32)


def test_small_hand_built_batch_on_device():
    from gcc_amd.encoder import GatEngine

    enc = gat_encoder(hidden=48, heads=4, layers=3, T=3, Lr=2, pos=16, deg_emb=8, max_degree=8).cuda()
    batch = symmetric_batch([6, 0, 1, 900], pos_dim=16, p=0.004, seed=3, isolated=(3,), extra_star=(3, 700))

    class G:
        pass

    g = G()
    n = int(batch["node_off"][-1])
    g.batch_size = 4
    g.node_off = batch["node_off"].int().cuda()
    g.row_ptr = torch.cat([batch["row_ptr"], batch["row_ptr"][-1:].repeat(50)]).int().cuda()     # capacity + 1 entries
    g.col_idx = batch["col_idx"].int().cuda()
    g.graph_id = torch.zeros(n + 50, dtype=torch.int32, device="cuda")
    g.pos_undirected = torch.cat([batch["pos_undirected"], torch.zeros(50, 16)]).cuda()
    dout = torch.randn(4, 48).cuda()
    out, grads, _ = kernel_grads(enc, GatEngine(), g, dout)
    ref_out, ref_grads = reference(enc, batch, dout.cpu())
    torch.testing.assert_close(out.double().cpu(), ref_out, rtol=1e-4, atol=1e-4)
    worst, name = worst_rel(grads, ref_grads)
    assert worst < 1e-3, (worst, name)


def test_test_moco_embeds_the_mean_of_both_views():
    """gcc_amd.generate.test_moco (generate.py:33-53) on a GAT model: (f(q) + f(k)) / 2 of the float64 restatement, view by
    view (a q-only embedding or a wrong pairing would not match)"""
    from gcc_amd.generate import test_moco
    from tests.gat_check import params_of

    q, hq, k, hk = _sampled_batch(B=64, hops=64, both=True)
    q.valid = q.batch_size
    enc = gat_encoder().cuda()
    emb = test_moco([(q, k)], enc, lambda v: None)
    with torch.no_grad():
        P = params_of(enc)
        want = (forward_of(enc, P, hq, **_seed_kw(q)) + forward_of(enc, P, hk, **_seed_kw(k))) / 2
    torch.testing.assert_close(emb.double(), want, rtol=1e-4, atol=1e-5)


def test_reference_fixture_on_device():
    """tests/golden/gat_golden.pt (the reference's own code) through the kernels on the device"""
    from gcc_amd.encoder import GatEngine
    from tests.gat_check import check_golden_step, golden_encoder, load_golden

    gold = load_golden()
    enc = golden_encoder(gold).cuda()

    class G:
        pass

    def run(enc, batch, mult, dout):
        g = G()
        n = int(batch["node_off"][-1])
        g.batch_size = len(batch["node_off"]) - 1
        g.node_off = batch["node_off"].int().cuda()
        g.row_ptr = torch.cat([batch["row_ptr"], batch["row_ptr"][-1:].repeat(16)]).int().cuda()
        g.col_idx = batch["col_idx"].int().cuda()
        g.graph_id = torch.zeros(n + 16, dtype=torch.int32, device="cuda")
        g.pos_undirected = torch.cat([batch["pos_undirected"], torch.zeros(16, batch["pos_undirected"].shape[1])]).cuda()
        g.edge_multiplicity = mult
        if dout is None:
            out, _s, _p, _w = GatEngine().forward(enc, g)
            return out.cpu(), None
        out, grads, _ = kernel_grads(enc, GatEngine(), g, dout.cuda())
        return out.cpu(), {kk: v.cpu() for kk, v in grads.items()}

    for step in gold["steps"]:
        check_golden_step(enc, step, gold, run)


def _corpus(tmp_path):
    from gcc_amd import ingest
    from gcc_amd.graphgen import powerlaw_graph

    gs = [powerlaw_graph(20000, 200000, 0), powerlaw_graph(2500, 20000, 2)]
    sizes = np.array([len(rp) - 1 for rp, _ in gs], dtype=np.int64)
    path = tmp_path / "small.bin"
    ingest.write_dgl_graphs(str(path), gs, labels={"graph_sizes": sizes})
    return str(path), gs


@pytest.mark.parametrize("flags,tag", [(["--moco", "--nce-k", "256"], "gat-moco"), (["--nce-k", "31"], "gat-e2e")])
def test_train_py_model_gat_then_generate(tmp_path, flags, tag):
    import generate
    import train

    corpus, gs = _corpus(tmp_path)
    argv = ["--exp", tag, "--model", "gat", "--model-path", str(tmp_path / "s"), "--tb-path", str(tmp_path / "t"), "--gpu", "0",
            "--batch-size", "32", "--num-workers", "1", "--num-copies", "1", "--num-samples", "128", "--rw-hops", "64",
            "--dgl-file", corpus, "--epochs", "2", "--print-freq", "2", "--tb-freq", "1000"]
    args = train.parse_option(argv + flags)
    args.gpu = args.gpu[0]
    buf = io.StringIO()
    with redirect_stdout(buf):
        loss = train.main(args)
    vals = [float(l.split("loss ")[1].split(" ")[0]) for l in buf.getvalue().splitlines() if l.startswith("Train:")]
    assert len(vals) == 4 and all(np.isfinite(v) for v in vals), vals
    assert np.isfinite(loss)
    path = os.path.join(args.model_folder, "current.pth")
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert "gnn.layers.0.gnn.attn_l" in ckpt["model"] and "set2set.lstm.weight_ih_l2" in ckpt["model"]
    fresh = gat_encoder()
    fresh.load_state_dict(ckpt["model"], strict=True)
    if "--moco" not in flags:
        return
    rp, ci = gs[1]
    npz = tmp_path / "g.npz"
    np.savez(npz, row_ptr=rp, col_idx=ci)
    a = types.SimpleNamespace(load_path=path, dataset="toy", gpu=0, edgelist=None, nodelabel=None, graph_npz=str(npz),
                              graphs_npz=None, tudataset=None, edge_multiplicity=1, batch_size=64)
    generate.main(a)
    emb = np.load(os.path.join(args.model_folder, "toy.npy"))
    assert emb.shape == (len(rp) - 1, 64) and np.isfinite(emb).all()
    norms = np.linalg.norm(emb, axis=1)
    assert norms.max() <= 1.0 + 1e-4 and norms.min() > 0.05        # mean of two unit vectors


def test_train_py_finetune_model_gat(tmp_path):
    import train
    from gcc_amd.contrast import MemoryMoCo
    from gcc_amd.graphgen import powerlaw_graph

    opt = train.parse_option(["--model-path", str(tmp_path / "saved"), "--tb-path", str(tmp_path / "tb"), "--moco",
                              "--nce-k", "64", "--rw-hops", "32", "--num-layer", "3", "--max-degree", "64", "--model", "gat"])
    enc = gat_encoder(layers=3, max_degree=64, seed=3)
    ckpt = tmp_path / "pretrained.pth"
    torch.save({"opt": opt, "model": enc.state_dict(), "contrast": MemoryMoCo(64, None, 64, 0.07, use_softmax=True).state_dict(),
                "optimizer": {}, "epoch": 1}, ckpt)
    rps, cis, labels = [], [], []
    for i in range(40):
        rp, ci = powerlaw_graph(12 + (i % 7) * 3, 40 + (i % 5) * 10, 100 + i)
        rps.append(rp)
        cis.append(ci)
        labels.append(i % 3)
    node_off = np.concatenate([[0], np.cumsum([len(rp) - 1 for rp in rps])])
    edge_base = np.concatenate([[0], np.cumsum([len(ci) for ci in cis])])
    row_ptr = np.concatenate([[0]] + [rp[1:] + edge_base[i] for i, rp in enumerate(rps)])
    npz = tmp_path / "graphs.npz"
    np.savez(npz, node_off=node_off, row_ptr=row_ptr, col_idx=np.concatenate(cis), graph_labels=np.array(labels))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--finetune", "--resume", str(ckpt), "--dataset",
                        "imdb-binary", "--epochs", "2", "--batch-size", "16", "--graphs-npz", str(npz), "--gpu", "0"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"Epoch 2, loss ([0-9.naninf]+), f1 ([0-9.]+)", r.stdout)
    assert m and np.isfinite(float(m.group(1))), r.stdout[-2000:]
