"""Fine-tuning (train.py --finetune [--cv]) on a real MI355X: the reference golden through the C ABI with the producer stream
off and on, run-to-run bit identity, and train.py end to end on a labelled edge list and on a set of labelled small graphs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("prefetch", [False, True])
def test_finetune_golden_on_device(prefetch):
    from tests.finetune_check import check_eval, check_steps, run_steps

    model, head, step, outs = run_steps("cuda:0", prefetch=prefetch)
    torch.cuda.synchronize()
    check_steps(model, step, outs)
    check_eval(model, head, "cuda:0")


def test_finetune_two_runs_are_bit_identical():
    """The head's reductions run in a fixed order: identical inputs give bit-identical loss, logits, dlogits, dW / db and
    dfeat.  (The encoder backward accumulates its BatchNorm statistics gradients with float atomics, so the encoder's
    flat gradient -- and hence everything after the first Adam step -- is compared by tests/finetune_check.py's bounds.)"""
    from tests.finetune_check import run_steps

    res = []
    for _ in range(2):
        model, head, step, outs = run_steps("cuda:0", prefetch=True)
        torch.cuda.synchronize()
        res.append(outs[0])
    for k in ("loss", "logits", "dlogits", "correct", "feat", "hgrad"):
        assert torch.equal(res[0][k], res[1][k]), k
    from gcc_amd.finetune import ClsHeadEngine

    g = torch.Generator().manual_seed(11)
    feat, W, b = torch.randn(256, 64, generator=g).cuda(), torch.randn(5, 64, generator=g).cuda(), torch.randn(5, generator=g).cuda()
    y = torch.randint(0, 5, (256,), generator=g, dtype=torch.int32).cuda()
    outs = []
    for _ in range(2):
        dW, db, dfeat = torch.empty(5, 64, device="cuda"), torch.empty(5, device="cuda"), torch.empty(256, 64, device="cuda")
        o = ClsHeadEngine().train(feat, W, b, y, dW, db, dfeat)
        outs.append((o["loss"].cpu(), dW.cpu(), db.cpu(), dfeat.cpu()))
    for a, c in zip(*outs):
        assert torch.equal(a, c)


@pytest.mark.parametrize("B,C,D", [(1024, 64, 256), (256, 5, 64), (33, 2, 128)])
def test_head_large_shapes_match_float64(B, C, D):
    from gcc_amd.finetune import ClsHeadEngine

    g = torch.Generator().manual_seed(B + C + D)
    feat, W, b = torch.randn(B, D, generator=g), torch.randn(C, D, generator=g) * 0.2, torch.randn(C, generator=g)
    y = torch.randint(0, C, (B,), generator=g, dtype=torch.int32)
    y[-3:] = -1
    dev = "cuda:0"
    dW, db, dfeat = torch.empty(C, D, device=dev), torch.empty(C, device=dev), torch.empty(B, D, device=dev)
    out = ClsHeadEngine().train(feat.to(dev), W.to(dev), b.to(dev), y.to(dev), dW, db, dfeat)
    v = y >= 0
    f, Wd, bd = feat.double().requires_grad_(), W.double().requires_grad_(), b.double().requires_grad_()
    loss = torch.nn.functional.cross_entropy((f @ Wd.t() + bd)[v], y[v].long())
    loss.backward()
    torch.testing.assert_close(out["loss"].cpu().double().reshape(()), loss.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(dW.cpu().double(), Wd.grad, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(db.cpu().double(), bd.grad, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(dfeat.cpu().double(), f.grad, rtol=1e-4, atol=1e-6)


def _checkpoint(tmp_path):
    """a tiny "pre-trained" checkpoint in the reference's format ({opt, model, contrast, optimizer, epoch})"""
    import train
    from gcc_amd.contrast import MemoryMoCo
    from gcc_amd.encoder import GraphEncoder

    opt = train.parse_option(["--model-path", str(tmp_path / "saved"), "--tb-path", str(tmp_path / "tb"), "--moco",
                              "--nce-k", "64", "--rw-hops", "32", "--num-layer", "3", "--max-degree", "64"])
    torch.manual_seed(3)
    model = GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=64,
                         freq_embedding_size=16, degree_embedding_size=16, output_dim=64, node_hidden_dim=64,
                         edge_hidden_dim=64, num_layers=3, num_step_set2set=6, num_layer_set2set=3, norm=True,
                         gnn_model="gin", degree_input=True)
    contrast = MemoryMoCo(64, None, 64, 0.07, use_softmax=True)
    path = tmp_path / "pretrained.pth"
    torch.save({"opt": opt, "model": model.state_dict(), "contrast": contrast.state_dict(), "optimizer": {}, "epoch": 1}, path)
    return str(path)


def _run(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_train_py_finetune_on_a_labelled_edge_list(tmp_path):
    from gcc_amd.graphgen import powerlaw_graph

    rp, ci = powerlaw_graph(600, 3000, 5)
    rng = np.random.default_rng(0)
    with open(tmp_path / "g.edgelist", "w") as f:
        for u in range(len(rp) - 1):
            for v in ci[rp[u]:rp[u + 1]]:
                if u < v:
                    f.write(f"{u} {v}\n")
    with open(tmp_path / "g.nodelabel", "w") as f:
        for u in range(len(rp) - 1):
            f.write(f"{u} {rng.integers(0, 4)}\n")
    ckpt = _checkpoint(tmp_path)
    out = _run(["--finetune", "--resume", ckpt, "--dataset", "usa_airport", "--epochs", "2", "--batch-size", "32",
                "--edgelist", str(tmp_path / "g.edgelist"), "--nodelabel", str(tmp_path / "g.nodelabel"), "--gpu", "0",
                "--print-freq", "5"])
    m = re.search(r"Epoch 2, loss ([0-9.naninf]+), f1 ([0-9.]+)", out)
    assert m and np.isfinite(float(m.group(1))) and 0.0 <= float(m.group(2)) <= 1.0, out[-2000:]
    assert re.search(r"Train: \[2\]\[10/\d+\]", out), out[-2000:]          # (--print-freq comes from the checkpoint: the resume override)


def _graphs_npz(tmp_path, n=60):
    from gcc_amd.graphgen import powerlaw_graph

    rps, cis, labels = [], [], []
    for i in range(n):
        rp, ci = powerlaw_graph(12 + (i % 7) * 3, 40 + (i % 5) * 10, 100 + i)
        rps.append(rp)
        cis.append(ci)
        labels.append(i % 3)
    node_off = np.concatenate([[0], np.cumsum([len(rp) - 1 for rp in rps])])
    edge_base = np.concatenate([[0], np.cumsum([len(ci) for ci in cis])])
    row_ptr = np.concatenate([[0]] + [rp[1:] + edge_base[i] for i, rp in enumerate(rps)])
    path = tmp_path / "graphs.npz"
    np.savez(path, node_off=node_off, row_ptr=row_ptr, col_idx=np.concatenate(cis), graph_labels=np.array(labels))
    return str(path)


def test_train_py_cv_on_labelled_small_graphs(tmp_path):
    ckpt = _checkpoint(tmp_path)
    out = _run(["--finetune", "--cv", "--resume", ckpt, "--dataset", "imdb-binary", "--epochs", "1", "--batch-size", "16",
                "--graphs-npz", _graphs_npz(tmp_path), "--gpu", "0"], timeout=900)
    assert len(re.findall(r"Epoch 1, loss [0-9.]+, f1 [0-9.]+", out)) == 10
    m = re.search(r"^\[([^\]]*)\]$", out, flags=re.M)
    assert m and len(m.group(1).split(",")) == 10
    assert re.search(r"Mean = [0-9.]+; Std = [0-9.]+", out)
    # every fold starts from the checkpoint's weights: ten "loaded successfully" lines, one per fold
    assert out.count("=> loaded successfully") == 10


def test_each_fold_starts_from_the_checkpoint(tmp_path, capsys):
    """two main() calls in ONE process on the same fold give the same held-out result only if the second starts from the
    checkpoint again (nothing of the first fold's training survives into the next)"""
    import train

    ckpt = _checkpoint(tmp_path)
    npz = _graphs_npz(tmp_path)
    f1 = []
    for _ in range(2):
        args = train.parse_option(["--finetune", "--resume", ckpt, "--dataset", "imdb-binary", "--epochs", "2",
                                   "--batch-size", "16", "--graphs-npz", npz, "--gpu", "0", "--fold-idx", "3"])
        args.gpu = 0
        f1.append(train.main(args))
    lines = re.findall(r"Epoch 2, loss [0-9.]+, f1 [0-9.]+", capsys.readouterr().out)
    assert len(lines) == 2 and lines[0] == lines[1] and f1[0] == f1[1]
