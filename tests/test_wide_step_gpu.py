"""The fused any-width step (MoCoTrainStep._body over csrc/ginx.hip and the dense head) at --hidden-size 256 on a device-sampled
batch -- G1 (1M nodes / 10M edges), bsz 256, rw_hops 256, K 16384, positional embedding by the device eigensolvers -- against
oracle/encoder.py fed the same batch, dropout masks, weights, Adam moments and queue, in fp32 and in float64
(tests/wide_step_check.py).  At ~25 k live rows per view every weight gradient spans many 1,024-row slabs, and the checked step
is the second, so rows past its live count hold whatever the first step's batch left there.  The shape edges of the same kernels
(off-grid widths, partial tiles, stale rows in a hand-built batch, the head around its split) run on the device in
tests/test_wide_edges_gpu.py, the device tier of tests/test_wide_edges_emu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, K, HOPS, RESTART, RUN_SEED, HIDDEN = 256, 16384, 256, 0.8, 0, 256


def test_fused_wide_step_on_a_sampled_batch_vs_float64_oracle():
    from gcc_amd.contrast import MemoryMoCo
    from gcc_amd.graph import DeviceGraph
    from gcc_amd.graphgen import powerlaw_graph
    from gcc_amd.posemb import DevicePosEmb
    from gcc_amd.sampler import DeviceRWRSampler
    from gcc_amd.train_step import MoCoTrainStep
    from tests.test_wide_encoder_emu import wide_encoder
    from tests.wide_step_check import check_wide_moco_step

    rp, ci = powerlaw_graph(1_000_000, 10_000_000, seed=0)
    graph = DeviceGraph(rp, ci, rw_hops=HOPS, restart_prob=RESTART, device="cuda:0", validate=False, trusted=True)
    torch.manual_seed(256)
    model, ema = wide_encoder(HIDDEN, HIDDEN).cuda(), wide_encoder(HIDDEN, HIDDEN).cuda()
    ema.load_state_dict(model.state_dict())
    contrast = MemoryMoCo(HIDDEN, None, K, 0.07, use_softmax=True).cuda()
    smp = DeviceRWRSampler(graph, B, run_seed=RUN_SEED, num_buffers=2)
    pe = DevicePosEmb(B, smp.node_cap, 32, device="cuda:0", seed=RUN_SEED, num_buffers=2, max_views=2)
    tr = MoCoTrainStep(model, ema, contrast, smp, pe, prefetch=False)
    assert tr.wide and not tr.use_graph
    L = len(model.gnn.ginlayers)
    tr.step(0, 0.005)                                    # an ordinary first step (dropout masks from torch.rand)
    masks = (torch.rand(L + 1, B, HIDDEN) >= 0.5).float().cuda().contiguous()
    rep = check_wide_moco_step(tr, model, ema, contrast, 0.004, masks, sync=torch.cuda.synchronize, step_id=1)
    assert tr.check_status(strict_posemb=True) == 0
    assert rep["nodes_q"] > 10 * B and rep["nodes_k"] > 10 * B, rep          # a real batch (~ 25 k nodes per view)
    print(f"hidden {HIDDEN} fused step, worst gradient entry vs float64: {rep['grad_err_vs_f64_step']:.2e} of the tensor's largest "
          f"entry ({rep['grad_worst_tensor']}); torch fp32 on the same inputs: {rep['grad_err_vs_f64_torch32']:.2e}")
    worst5 = sorted(rep.pop("grad_err_by_tensor").items(), key=lambda kv: -kv[1][0])[:5]
    print("largest gradient errors vs float64 (step, torch fp32):", [(n, f"{a:.2e}", f"{b:.2e}") for n, (a, b) in worst5])
    print("report:", rep)
