"""The GAT path against tests/golden/gat_golden.pt, made by running the reference's own gat.py / graph_encoder.py /
MemoryMoCo / NCESoftmaxLoss (tests/golden/make_gat_golden.py): the float64 restatement reproduces the recorded forward,
loss and gradients; GraphEncoder(gnn_model="gat") loads the state_dict strictly and initialises exactly the recorded
weights under the same seed; the kernels (emulator build) reproduce the fixture."""
import torch

from gcc_amd.encoder import GatEngine, GraphEncoder
from tests.gat_check import check_golden_step, golden_encoder, kernel_grads, load_golden, moco_loss
from tests.gat_reference import forward_of, params_of
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_encoder import CpuBatch


def test_restatement_reproduces_the_reference():
    gold = load_golden()
    enc = golden_encoder(gold)
    for step in gold["steps"]:
        P = params_of(enc)
        fq = forward_of(enc, P, step["q"], mult=step["edge_multiplicity"])
        with torch.no_grad():
            fk = forward_of(enc, params_of(enc), step["k"], mult=step["edge_multiplicity"])
        loss = moco_loss(fq, fk, step["memory"].double(), gold["nce_t"])
        loss.backward()
        torch.testing.assert_close(fq.detach().float(), step["feat_q"], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(fk.float(), step["feat_k"], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(loss.float(), step["loss"], rtol=1e-5, atol=1e-6)
        for k, g in step["grads"].items():
            scale = float(g.abs().max())
            assert float((P[k].grad - g.double()).abs().max()) <= 1e-4 * scale + 1e-9, k


def test_strict_load_and_initial_weights_equal_the_references():
    gold = load_golden()
    torch.manual_seed(gold["seed"])
    enc = GraphEncoder(**gold["cfg"])
    sd = enc.state_dict()
    assert set(sd) == set(gold["init"])
    for k, v in gold["init"].items():
        assert torch.equal(sd[k], v), k                      # set2set.* and lin_readout.* included
    GraphEncoder(**gold["cfg"]).load_state_dict(gold["init"], strict=True)


def _emu_run(enc, batch, mult, dout):
    eng = GatEngine(lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr())
    g = CpuBatch(batch)
    g.edge_multiplicity = mult
    if dout is None:
        out, _saved, _p, _w = eng.forward(enc, g)
        return out, None
    out, grads, _ = kernel_grads(enc, eng, g, dout)
    return out, grads


def test_kernels_reproduce_the_reference_on_the_emulator():
    gold = load_golden()
    enc = golden_encoder(gold)
    for step in gold["steps"]:
        check_golden_step(enc, step, gold, _emu_run)
