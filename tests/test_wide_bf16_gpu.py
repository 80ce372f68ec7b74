"""Device tier of tests/test_wide_bf16_emu.py: ``--encoder-dtype bf16 --nce-dtype bf16`` on the GPU.

* The fused any-width step at --hidden-size 256 on a device-sampled batch -- G1 (1M nodes / 10M edges), bsz 256, rw_hops 256,
  K 16384, positional embedding by the device eigensolvers, the setup of tests/test_wide_step_gpu.py -- with both dtypes bf16:
  the SECOND step against the rounded oracle of tests/bf16_reference.py in float64 (tests/wide_bf16_step_check.py), at the
  emulator tier's bars.  ~25 k live rows per view: every weight gradient spans ~25 split-K slabs of the bf16 kernel.
* train.py --hidden-size 128 --encoder-dtype bf16 --nce-dtype bf16 for a few steps, then generate.py on its checkpoint.

Measured on an MI355X (second step, 5 layers, hidden 256; err = the step, gap = the rounded oracle's fp32 run, both against
its float64 run, in the unit of each bar; 22,654 + 22,592 nodes): embeddings err 3.59e-04 | gap 6.60e-04; loss / prob / gradient
norm 1.42e-03 | 1.14e-03; gradients 8.14e-02 | 8.21e-02; running statistics 9.86e-02 | 1.35e-01; model_ema 4.09e-02 | 5.58e-02.
Step times: DESIGN.md 4f."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, K, HOPS, RESTART, RUN_SEED, HIDDEN = 256, 16384, 256, 0.8, 0, 256


def test_fused_wide_bf16_step_on_a_sampled_batch_vs_rounded_float64_oracle():
    from gcc_amd.contrast import MemoryMoCo
    from gcc_amd.graph import DeviceGraph
    from gcc_amd.graphgen import powerlaw_graph
    from gcc_amd.posemb import DevicePosEmb
    from gcc_amd.sampler import DeviceRWRSampler
    from gcc_amd.train_step import MoCoTrainStep
    from tests.test_wide_bf16_emu import wide_encoder
    from tests.wide_bf16_step_check import check_wide_bf16_moco_step

    rp, ci = powerlaw_graph(1_000_000, 10_000_000, seed=0)
    graph = DeviceGraph(rp, ci, rw_hops=HOPS, restart_prob=RESTART, device="cuda:0", validate=False, trusted=True)
    torch.manual_seed(256)
    model, ema = wide_encoder(HIDDEN, HIDDEN, encoder_dtype="bf16").cuda(), wide_encoder(HIDDEN, HIDDEN, encoder_dtype="bf16").cuda()
    ema.load_state_dict(model.state_dict())
    contrast = MemoryMoCo(HIDDEN, None, K, 0.07, use_softmax=True, nce_dtype="bf16").cuda()
    smp = DeviceRWRSampler(graph, B, run_seed=RUN_SEED, num_buffers=2)
    pe = DevicePosEmb(B, smp.node_cap, 32, device="cuda:0", seed=RUN_SEED, num_buffers=2, max_views=2)
    tr = MoCoTrainStep(model, ema, contrast, smp, pe, prefetch=False)
    assert tr.wide and not tr.use_graph and tr.nce.dtype == "bf16"
    L = len(model.gnn.ginlayers)
    tr.step(0, 0.005)                                    # an ordinary first step (dropout masks from torch.rand)
    masks = (torch.rand(L + 1, B, HIDDEN) >= 0.5).float().cuda().contiguous()
    rep = check_wide_bf16_moco_step(tr, model, ema, contrast, 0.004, masks, sync=torch.cuda.synchronize, step_id=1)
    assert tr.check_status(strict_posemb=True) == 0
    assert rep["nodes_q"] > 10 * B and rep["nodes_k"] > 10 * B, rep          # a real batch (~ 25 k nodes per view)
    print(f"hidden {HIDDEN} fused bf16 step: " + rep.pop("bars").summary())
    print("report:", rep)


def test_train_py_bf16_hidden_128_then_generate(tmp_path):
    import io
    from contextlib import redirect_stdout

    import generate
    import train
    from tests.test_train_main_gpu import _corpus

    corpus, gs = _corpus(tmp_path)
    argv = ["--exp", "widebf16", "--model-path", str(tmp_path / "s"), "--tb-path", str(tmp_path / "t"), "--gpu", "0", "--moco", "--nce-k", "256",
            "--hidden-size", "128", "--encoder-dtype", "bf16", "--nce-dtype", "bf16", "--batch-size", "32", "--num-workers", "2",
            "--num-copies", "1", "--num-samples", "256", "--rw-hops", "64", "--dgl-file", corpus, "--epochs", "2", "--print-freq", "4",
            "--tb-freq", "1000"]
    args = train.parse_option(argv)
    args.gpu = args.gpu[0]
    buf = io.StringIO()
    with redirect_stdout(buf):
        loss = train.main(args)
    vals = [float(l.split("loss ")[1].split(" ")[0]) for l in buf.getvalue().splitlines() if l.startswith("Train:")]
    assert len(vals) == 8 and all(np.isfinite(v) and 0.0 < v < 7.0 for v in vals), vals      # 2 epochs x 16 steps / 4
    # model_name is unchanged by the two dtype flags: the same argv without them names the same folder
    plain = train.option_update(train.parse_option([a for a in argv if a not in ("--encoder-dtype", "--nce-dtype", "bf16")]))
    assert plain.encoder_dtype == "f32" and plain.nce_dtype == "f32"
    assert np.isfinite(loss) and "_hid_128_" in os.path.basename(args.model_folder)
    assert os.path.basename(args.model_folder) == args.model_name == plain.model_name
    ckpt = torch.load(os.path.join(args.model_folder, "current.pth"), map_location="cpu", weights_only=False)
    assert ckpt["opt"].encoder_dtype == "bf16" and ckpt["opt"].nce_dtype == "bf16"
    assert ckpt["contrast"]["memory"].shape == (256, 128)
    assert ckpt["model"]["gnn.ginlayers.1.apply_func.mlp.linears.0.weight"].shape == (128, 128)
    rp, ci = gs[2]
    npz = tmp_path / "g.npz"
    np.savez(npz, row_ptr=rp, col_idx=ci)
    a = types.SimpleNamespace(load_path=os.path.join(args.model_folder, "current.pth"), dataset="toy", gpu=0, edgelist=None,
                              nodelabel=None, graph_npz=str(npz), graphs_npz=None, tudataset=None, edge_multiplicity=2, batch_size=64)
    generate.main(a)
    emb = np.load(os.path.join(args.model_folder, "toy.npy"))
    assert emb.shape == (len(rp) - 1, 128) and np.isfinite(emb).all()
    # generate.py:48-52 writes (f(q) + f(k)) / 2 of two unit-norm views (graph_encoder.py:195-196): inside the unit ball, not at 0
    norms = np.linalg.norm(emb, axis=1)
    assert (norms <= 1.0 + 1e-4).all() and (norms > 0.1).all(), (norms.min(), norms.max())
    # ... and each view's embedding is unit-norm: the checkpoint's encoder, rebuilt as generate.py rebuilds it, on a sampled batch
    from gcc_amd.encoder import encoder_from_opt
    from gcc_amd.graph import DeviceGraph
    from gcc_amd.posemb import DevicePosEmb
    from gcc_amd.sampler import DeviceRWRSampler

    enc = encoder_from_opt(ckpt["opt"]).cuda()
    assert enc.wide and enc.encoder_dtype == "bf16"
    enc.load_state_dict(ckpt["model"])
    enc.eval()
    smp = DeviceRWRSampler(DeviceGraph(rp, ci, rw_hops=64, device="cuda:0"), batch_size=32, run_seed=1)
    q, k = smp.sample(0)
    smp.check_status()
    pe = DevicePosEmb(32, smp.node_cap, 32, device="cuda:0", seed=1)
    pe(q)
    pe(k)
    with torch.no_grad():
        for view in (q, k):
            feat = enc(view)
            assert feat.shape == (32, 128) and bool(torch.isfinite(feat).all())
            torch.testing.assert_close(feat.norm(dim=1), torch.ones(32, device="cuda"), rtol=0, atol=1e-4)
