"""Generates tests/golden/finetune_golden.pt by EXECUTING THE REFERENCE'S OWN GraphEncoder (gcc/models/{gin,graph_encoder}.py,
with DGL replaced by tests/golden/dgl_stub.py) inside the reference's fine-tuning step (train_finetune, train.py:175-297):
nn.Linear(64, 3) head, nn.CrossEntropyLoss, clip_grad_value_(..., 1) on both, two torch.optim.Adam with the
warmup_linear(., 0.1) learning rate, clear_bn before the first step; then one test_finetune pass (train.py:300-337).  Run
from the repo root:

    python tests/golden/make_finetune_golden.py

Two consecutive steps (the Adam moments matter); the second batch is partial (4 graphs where the first has 6).  Records the
inputs, labels, initial weights, dropout keep-masks, logits, losses, predictions, post-clip gradients, post-step weights
(BatchNorm running statistics included) and the eval logits / loss / F1.  Tensors only.
"""
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_encoder_golden as M  # noqa: E402  (installs the DGL stub, puts the reference on sys.path)

from gcc.utils.misc import warmup_linear  # noqa: E402

dgl_stub = M.dgl_stub


def sd(module):
    # set2set.* / lin_readout.* are allocated but never used on the GIN path (no gradient, Adam leaves them): not recorded
    return {k: v.clone() for k, v in module.state_dict().items() if not k.startswith(("set2set.", "lin_readout."))}


def build_encoder():
    # train.py:601-620 with --num-layer 3 and a max degree of 64: a small model keeps the fixture well under 1 MB
    from gcc.models import GraphEncoder

    return GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=64,
                        freq_embedding_size=16, degree_embedding_size=16, output_dim=64, node_hidden_dim=64,
                        edge_hidden_dim=64, num_layers=3, num_step_set2set=6, num_layer_set2set=3,
                        norm=True, gnn_model="gin", degree_input=True)


def main():
    gen = torch.Generator().manual_seed(4321)
    batches = [M.make_inputs(B=6, rw_hops=32, run_seed=5)[0], M.make_inputs(B=4, rw_hops=32, run_seed=9)[0]]
    labels = [torch.randint(0, 3, (6,), generator=gen), torch.randint(0, 3, (4,), generator=gen)]
    torch.manual_seed(0)
    model = build_encoder()
    head = nn.Linear(64, 3)
    with torch.no_grad():                          # non-trivial BN parameters and running statistics (clear_bn must reset them)
        for m in model.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5, generator=gen)
                m.bias.uniform_(-0.3, 0.3, generator=gen)
                m.running_mean.uniform_(-1, 1, generator=gen)
                m.running_var.uniform_(0.5, 2, generator=gen)
                m.num_batches_tracked.fill_(7)
    init = dict(model=sd(model), head=sd(head))

    def clear_bn(m):                               # train.py:651-655
        if m.__class__.__name__.find("BatchNorm") != -1:
            m.reset_running_stats()

    model.apply(clear_bn)
    criterion = nn.CrossEntropyLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=0.005, betas=(0.9, 0.999), weight_decay=1e-5)
    head_optimizer = torch.optim.Adam(head.parameters(), lr=0.005, betas=(0.9, 0.999), weight_decay=1e-5)
    model.gnn.drop = M.RecordedDropout(0.5, gen)
    epochs, n_batch, epoch = 10, 2, 1
    steps = []
    for idx, (view, y) in enumerate(zip(batches, labels)):
        model.train()
        head.train()
        g = dgl_stub.StubBatchedGraph(**view)
        n_masks = len(model.gnn.drop.masks)
        feat_q = model(g)
        out = head(feat_q)
        loss = criterion(out, y)
        optimizer.zero_grad()
        head_optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_value_(model.parameters(), 1)
        torch.nn.utils.clip_grad_value_(head.parameters(), 1)
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None and not n.startswith("set2set.")}
        head_grads = {n: p.grad.clone() for n, p in head.named_parameters()}
        global_step = epoch * n_batch + idx
        lr = 0.005 * warmup_linear(global_step / (epochs * n_batch), 0.1)
        for opt in (optimizer, head_optimizer):
            for pg in opt.param_groups:
                pg["lr"] = lr
        optimizer.step()
        head_optimizer.step()
        steps.append(dict(lr=lr, masks=torch.stack(model.gnn.drop.masks[n_masks:]), feat=feat_q.detach(),
                          logits=out.detach(), loss=loss.detach(), preds=out.argmax(1), grads=grads, head_grads=head_grads,
                          model=sd(model), head=sd(head)))
    # test_finetune over the two batches (a held-out loader of 6 + 4 items)
    model.eval()
    head.eval()
    ev_logits, loss_sum, f1_sum, n = [], 0.0, 0.0, 0
    for view, y in zip(batches, labels):
        g = dgl_stub.StubBatchedGraph(**view)
        with torch.no_grad():
            out = head(model(g))
        loss = criterion(out, y)
        f1 = float((out.argmax(1) == y).double().mean())     # f1_score(average="micro") of single-label multiclass
        ev_logits.append(out)
        loss_sum += float(loss) * g.batch_size
        f1_sum += f1 * g.batch_size
        n += g.batch_size
    gold = dict(config=dict(num_layers=3, max_degree=64), batches=batches, labels=labels, init=init, steps=steps,
                eval=dict(logits=ev_logits, loss=torch.tensor(loss_sum / n), f1=torch.tensor(f1_sum / n)))
    path = os.path.join(HERE, "finetune_golden.pt")
    torch.save(gold, path)
    print("wrote", path, os.path.getsize(path), "bytes; losses", [float(s["loss"]) for s in steps],
          "eval", float(gold["eval"]["loss"]), float(gold["eval"]["f1"]))


if __name__ == "__main__":
    main()
