"""Shared body of the fine-tuning golden tests (tests/test_finetune_emu.py on the emulator build, tests/test_finetune_gpu.py on
the device): FinetuneTrainStep + evaluate() against tests/golden/finetune_golden.pt, which was produced by executing the
reference's GraphEncoder inside the reference's train_finetune / test_finetune."""
import os

import numpy as np
import torch
import torch.nn as nn

from gcc_amd.encoder import GraphEncoder
from gcc_amd.finetune import FinetuneTrainStep, LabeledProducer, clear_bn, evaluate
from tests.hipemu.emu_encoder import CpuBatch

GOLD = torch.load(os.path.join(os.path.dirname(__file__), "golden", "finetune_golden.pt"), weights_only=False)
B = 6          # the first batch's size; the second (4 graphs) is padded with empty subgraphs to it


def golden_encoder():
    cfg = GOLD["config"]
    return GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=cfg["max_degree"],
                        freq_embedding_size=16, degree_embedding_size=16, output_dim=64, node_hidden_dim=64,
                        edge_hidden_dim=64, num_layers=cfg["num_layers"], num_step_set2set=6, num_layer_set2set=3,
                        norm=True, gnn_model="gin", degree_input=True)


def padded_view(view):
    """the golden batch padded to B rows with empty subgraphs (flat node_off tail), as the labelled datasets pad"""
    v = dict(view)
    no = view["node_off"]
    v["node_off"] = torch.cat([no, no[-1:].repeat(B + 1 - len(no))])
    return v


def batch(i, device):
    g = CpuBatch(padded_view(GOLD["batches"][i]))
    g.edge_multiplicity = 1
    if device != "cpu":
        for name in ("node_off", "row_ptr", "col_idx", "edge_off", "graph_id", "parent_nid", "pos_undirected"):
            setattr(g, name, getattr(g, name).to(device))
    y = torch.full((B,), -1, dtype=torch.int32)
    y[: len(GOLD["labels"][i])] = GOLD["labels"][i].to(torch.int32)
    return g, y.to(device)


def padded_masks(i):
    m = GOLD["steps"][i]["masks"]                     # [L + 1, rows, 64]
    out = torch.zeros(m.shape[0], B, 64)
    out[:, : m.shape[1]] = m
    return out.contiguous()


class GoldenDataset:
    """the two golden batches behind the labelled datasets' make_batch / batches interface: item i IS golden batch i"""
    batch_size = 1                                     # (items per make_batch call)

    def __init__(self, device):
        self.device = device

    def make_batch(self, idx):
        return batch(int(idx[0]), self.device)

    def batches(self, order):
        for i in order:
            yield self.make_batch([i])


def make_model(device, gin_engine=None, head_engine=None):
    model, head = golden_encoder(), nn.Linear(64, 3)
    missing, unexpected = model.load_state_dict(GOLD["init"]["model"], strict=False)
    assert not unexpected and all(k.startswith(("set2set.", "lin_readout.")) for k in missing)
    head.load_state_dict(GOLD["init"]["head"])
    model, head = model.to(device), head.to(device)
    if gin_engine is not None:
        model._engine = gin_engine
    step = FinetuneTrainStep(model, head, learning_rate=0.005, betas=(0.9, 0.999), weight_decay=1e-5, clip_value=1.0,
                             engine=head_engine)
    clear_bn(model)                                    # after the re-homing: the buffers the kernels read are the ones reset
    return model, head, step


def run_steps(device, gin_engine=None, head_engine=None, prefetch=False):
    model, head, step = make_model(device, gin_engine, head_engine)
    outs, k = [], [0]

    def masks():
        m = padded_masks(k[0]).to(device)
        k[0] += 1
        return m

    step.mask_fn = masks
    prod = LabeledProducer(GoldenDataset(device), device, prefetch=prefetch)
    for i, (g, y) in enumerate(prod.batches([0, 1])):
        out = step.step(i, g, y, GOLD["steps"][i]["lr"])
        outs.append({kk: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for kk, v in out.items()})
        outs[-1]["flat_grad"] = step.flat_grad.detach().cpu().clone()
        outs[-1]["hgrad"] = step.hgrad.detach().cpu().clone()
        outs[-1]["model"] = {kk: v.detach().cpu().clone() for kk, v in model.state_dict().items()}
        outs[-1]["head"] = {kk: v.detach().cpu().clone() for kk, v in head.state_dict().items()}
    return model, head, step, outs


def check_steps(model, step, outs):
    from gcc_amd.encoder import grad_params

    names = dict(model.named_parameters())
    ids = {id(p): n for n, p in names.items()}
    assert len(outs) == len(GOLD["steps"])
    for i, (o, gs) in enumerate(zip(outs, GOLD["steps"])):
        rows = len(GOLD["labels"][i])
        torch.testing.assert_close(o["logits"][:rows], gs["logits"], rtol=1e-4, atol=2e-5, msg=f"step {i} logits")
        torch.testing.assert_close(o["loss"].reshape(()), gs["loss"], rtol=1e-4, atol=1e-5, msg=f"step {i} loss")
        assert torch.equal(o["logits"][:rows].argmax(1), gs["preds"]), i
        assert int(o["correct"][0]) == int((gs["preds"] == GOLD["labels"][i]).sum()) and int(o["correct"][1]) == rows
        assert torch.all(o["dlogits"][rows:] == 0)
        # post-clip gradients (the Adam launches leave the clipped gradient in the flat buffers, as torch leaves p.grad)
        off = 0
        for _, _, p in grad_params(model):
            n = ids[id(p)]
            got = o["flat_grad"][off:off + p.numel()].view_as(p)
            torch.testing.assert_close(got, gs["grads"][n], rtol=2e-3, atol=2e-6, msg=f"step {i} grad {n}")
            off += model.padded_numel(p)
        torch.testing.assert_close(o["hgrad"][:192].view(3, 64), gs["head_grads"]["weight"], rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(o["hgrad"][192:], gs["head_grads"]["bias"], rtol=1e-4, atol=1e-6)
        # post-step weights and BatchNorm running statistics
        for kk, v in gs["model"].items():
            got = o["model"][kk]
            g_ref = gs["grads"].get(kk)
            if g_ref is not None and i == 0:
                # a bias in front of a BatchNorm has a gradient of zero up to rounding (~1e-10): Adam's first step turns that
                # noise into +-lr, so such entries are held to the size of one step; every other entry to the usual bounds
                noise = g_ref.abs() < 1e-7
                assert torch.all((got - v).abs()[noise] <= 2 * gs["lr"]), f"step {i} {kk}"
                got, v = got[~noise], v[~noise]
            elif g_ref is not None:
                noise = (GOLD["steps"][0]["grads"][kk].abs() < 1e-7) | (g_ref.abs() < 1e-7)
                assert torch.all((got - v).abs()[noise] <= 2 * (gs["lr"] + GOLD["steps"][0]["lr"])), f"step {i} {kk}"
                got, v = got[~noise], v[~noise]
            torch.testing.assert_close(got, v, rtol=1e-3, atol=2e-5, msg=f"step {i} {kk}")
        for kk, v in gs["head"].items():
            torch.testing.assert_close(o["head"][kk], v, rtol=1e-4, atol=2e-6, msg=f"step {i} head {kk}")
    acc, mx = step.read_meters()
    n = sum(len(y) for y in GOLD["labels"])
    assert acc[2] == n and acc[4] == 2
    correct = sum(int((s["preds"] == y).sum()) for s, y in zip(GOLD["steps"], GOLD["labels"]))
    assert acc[1] == correct
    want = sum(float(s["loss"]) * len(y) for s, y in zip(GOLD["steps"], GOLD["labels"]))
    assert abs(acc[0] - want) < 1e-4 * n
    assert mx[0] == max(int(b["node_off"][-1]) for b in GOLD["batches"])


def check_eval(model, head, device, head_engine=None):
    loss, f1 = evaluate(model, head, GoldenDataset(device), [0, 1], engine=head_engine)
    assert abs(loss - float(GOLD["eval"]["loss"])) < 1e-4, (loss, float(GOLD["eval"]["loss"]))
    assert abs(f1 - float(GOLD["eval"]["f1"])) < 1e-6, (f1, float(GOLD["eval"]["f1"]))     # (the fixture holds it in float32)


def f1_micro(y, pred):
    return float(np.mean(np.asarray(y) == np.asarray(pred)))
