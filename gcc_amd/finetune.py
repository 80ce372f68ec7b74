"""Fine-tuning a pre-trained encoder on a labelled dataset: ``train_finetune`` / ``test_finetune`` of the reference's train.py
(:175-337) on the device.

    labelled batch (graph_q, labels) [producer stream, one batch ahead] -> GIN forward, train mode (in-kernel Philox dropout)
    -> head: Linear + CrossEntropy + backward + correct count (gcc_cls_head_train, one launch) -> GIN backward into the flat
    encoder gradient -> clip_grad_value_ + Adam over the encoder (gcc_adam_clipvalue_step) -> the same over the head's [W | b]

No host synchronisation inside a step: loss, correct predictions and graph sizes are accumulated on the device (the head's
launch updates the meters) and read when a log line is due.  The reference's two torch.optim.Adam (encoder and output layer,
same hyperparameters, same step count) are two launches over two flat buffers.
``--optimizer sgd`` / ``adagrad`` (with ``--step-path fused``) select the ENCODER's rule (gcc_opt_clipvalue_step, one launch as well);
the output layer's optimizer stays Adam, as in the reference (train.py:645-650).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _cabi
from .encoder import H
from .train_step import OPT_RULES, FlatRuleState, flat_grad_views, flatten_parameters


class ClsHeadEngine:
    """C-ABI calls of the head (csrc/cls_head.hip) and of the clip-by-value tail (csrc/step_tail.hip).  ``lib``/``ptr`` are
    injectable for the emulator tests only."""

    def __init__(self, lib=None, ptr=None):
        self.lib = lib if lib is not None else _cabi.load()
        self.ptr = ptr if ptr is not None else _cabi.dev_ptr

    def _args(self, feat, W, b, labels, ld_feat=None):
        B, C, D = int(labels.shape[0]), int(W.shape[0]), int(W.shape[1])
        if C > _cabi.CLS_HEAD_MAX_CLASSES or D > _cabi.CLS_HEAD_MAX_DIM:
            raise ValueError(f"the classifier head serves up to {_cabi.CLS_HEAD_MAX_CLASSES} classes and "
                             f"{_cabi.CLS_HEAD_MAX_DIM} features (got {C} x {D})")
        a = _cabi.GccClsHeadArgs()
        a.feat, a.W, a.b, a.labels = self.ptr(feat), self.ptr(W), self.ptr(b), self.ptr(labels)
        a.B, a.D, a.C = B, D, C
        a.ld_feat = int(ld_feat if ld_feat is not None else feat.shape[1])
        return a

    def train(self, feat, W, b, labels, dW, db, dfeat, logits=None, dlogits=None, meters=None, stream=None):
        """-> dict(loss [1], correct int32[2] {correct, valid}, logits, dlogits).  ``meters`` = (acc double[5], mx int32[2],
        graph): one step of the device-side meters."""
        B, C = int(labels.shape[0]), int(W.shape[0])
        f32 = dict(dtype=torch.float32, device=feat.device)
        out = dict(loss=torch.empty(1, **f32), correct=torch.empty(2, dtype=torch.int32, device=feat.device),
                   logits=logits if logits is not None else torch.empty(B, C, **f32),
                   dlogits=dlogits if dlogits is not None else torch.empty(B, C, **f32))
        a = self._args(feat, W, b, labels)
        a.ld_dfeat = int(dfeat.shape[1])
        a.logits, a.dlogits = self.ptr(out["logits"]), self.ptr(out["dlogits"])
        a.dW, a.db, a.dfeat, a.loss, a.correct = self.ptr(dW), self.ptr(db), self.ptr(dfeat), self.ptr(out["loss"]), self.ptr(out["correct"])
        if meters is not None:
            acc, mx, g = meters
            a.meter_acc, a.meter_max = self.ptr(acc), self.ptr(mx)
            a.node_off, a.edge_off = self.ptr(g.node_off), self.ptr(g.edge_off)
        _cabi.call(self.lib, "gcc_cls_head_train", ctypes.byref(a), stream)
        return out

    def eval(self, feat, W, b, labels, loss_sum, counts, logits=None, stream=None):
        """loss_sum (double[1]) += sum of the valid rows' CE, counts (int32[2]) += {correct, valid}"""
        a = self._args(feat, W, b, labels)
        a.logits = self.ptr(logits) if logits is not None else None
        a.eval_loss_sum, a.eval_counts = self.ptr(loss_sum), self.ptr(counts)
        _cabi.call(self.lib, "gcc_cls_head_eval", ctypes.byref(a), stream)

    def _clipvalue(self, rule, param, grad, states, lr, hyper, weight_decay, step, clip_value, grad_scale, stream):
        """one clip-by-value tail (csrc/step_tail.hip): ``rule`` None = Adam (``states`` = (exp_avg, exp_avg_sq), ``hyper`` =
        (beta1, beta2, eps), its ``step`` count), 1 = SGD (the momentum buffer; the momentum), 2 = Adagrad (the sum; eps)"""
        ptr = self.ptr
        _cabi.call(self.lib, "gcc_adam_clipvalue_step" if rule is None else "gcc_opt_clipvalue_step",
                   *([] if rule is None else [int(rule)]), ptr(param), ptr(grad), *(ptr(s) for s in states), param.numel(), lr, *hyper,
                   weight_decay, *([int(step)] if rule is None else []), clip_value, grad_scale, stream)

    def adam_clipvalue(self, param, grad, exp_avg, exp_avg_sq, lr, betas, eps, weight_decay, step, clip_value,
                       grad_scale=1.0, stream=None):
        self._clipvalue(None, param, grad, (exp_avg, exp_avg_sq), lr, (*betas, eps), weight_decay, step, clip_value, grad_scale, stream)

    def opt_clipvalue(self, rule, param, grad, state, lr, hyper, weight_decay, clip_value, grad_scale=1.0, stream=None):
        """gcc_opt_clipvalue_step: ``rule`` 1 = SGD (``state`` the momentum buffer, ``hyper`` the momentum), 2 = Adagrad (the sum
        of squares, eps; ``lr`` = the step's clr)"""
        self._clipvalue(int(rule), param, grad, (state,), lr, (hyper,), weight_decay, 0, clip_value, grad_scale, stream)


class _FlatClipValue(FlatRuleState):
    """clip_grad_value_(params, clip_value) + the rule's update over one flat buffer (train.py:232-246 of the reference), one
    launch: gcc_adam_clipvalue_step / gcc_opt_clipvalue_step"""

    def __init__(self, rule, param, grad, lr, weight_decay, clip_value, engine, **hyper):
        super().__init__(rule, param, grad, lr, weight_decay, engine, **hyper)
        self.clip_value = clip_value

    def step(self, stream=None):
        g = self.param_groups[0]
        self.steps += 1
        if self.rule == "adam":
            self.engine.adam_clipvalue(self.param, self.grad, *self.states, g["lr"], g["betas"], g["eps"], g["weight_decay"],
                                       self.steps, self.clip_value, stream=stream)
        else:
            self.engine.opt_clipvalue(OPT_RULES[self.rule], self.param, self.grad, self.state, self.rate(self.steps), self.hyper(),
                                      g["weight_decay"], self.clip_value, stream=stream)


class FlatAdamClipValue(_FlatClipValue):
    """clip_grad_value_ + torch.optim.Adam(lr, betas, eps=1e-8, weight_decay) (train.py:232-246,667-672 of the reference)"""

    def __init__(self, param, grad, lr, betas, weight_decay, clip_value, engine, eps=1e-8):
        super().__init__("adam", param, grad, lr, weight_decay, clip_value, engine, betas=betas, eps=eps)


class FlatSGDClipValue(_FlatClipValue):
    """clip_grad_value_ + torch.optim.SGD(lr, momentum, weight_decay) (train.py:232-246,658-666 of the reference)"""

    def __init__(self, param, grad, lr, momentum, weight_decay, clip_value, engine):
        super().__init__("sgd", param, grad, lr, weight_decay, clip_value, engine, momentum=momentum)


class FlatAdagradClipValue(_FlatClipValue):
    """clip_grad_value_ + torch.optim.Adagrad(lr, lr_decay, weight_decay) (train.py:232-246,673-679 of the reference)"""

    def __init__(self, param, grad, lr, lr_decay, weight_decay, clip_value, engine, eps=1e-10):
        super().__init__("adagrad", param, grad, lr, weight_decay, clip_value, engine, lr_decay=lr_decay, eps=eps)


def clear_bn(model):
    """train.py:651-655 of the reference: reset every BatchNorm's running statistics.  In place, so the buffers the kernels
    read (their padded homes after ``flatten_parameters``) are the ones reset."""
    for m in model.modules():
        if m.__class__.__name__.find("BatchNorm") != -1:
            m.reset_running_stats()


def flatten_head(head: nn.Linear):
    """Re-home the head's weight and bias into one flat buffer [W | b] (torch layout); -> (flat, flat gradient, dW, db)."""
    if getattr(head, "_flat", None) is None:
        W, b = head.weight, head.bias
        n = W.numel()
        flat = torch.empty(n + b.numel(), dtype=torch.float32, device=W.device)
        with torch.no_grad():
            flat[:n].copy_(W.reshape(-1))
            flat[n:].copy_(b)
        W.data = flat[:n].view_as(W)
        b.data = flat[n:]
        grad = torch.zeros_like(flat)
        head._flat, head._flat_grad = flat, grad
        head._dW, head._db = grad[:n].view_as(W), grad[n:]
    return head._flat, head._flat_grad, head._dW, head._db


def _meter_buffers(dev):
    """acc double[5]: sums of loss * valid, correct, valid rows, nodes, steps; mx int32[2]: max nodes / edges of a batch"""
    return torch.zeros(5, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)


class FinetuneTrainStep:
    """One step of train_finetune (train.py:204-246 of the reference) as a fixed sequence of launches on the step stream.
    ``model`` must be a GraphEncoder served by the fused 64-channel kernels (hidden size up to 64); wider models
    take the API path (:func:`api_step`).  ``optimizer``: the ENCODER's -- "adam", "sgd" (``momentum``) or "adagrad"
    (``lr_decay``); the head's stays Adam, as in the reference (train.py:645-650)."""

    def __init__(self, model, head: nn.Linear, learning_rate=0.005, betas=(0.9, 0.999), weight_decay=1e-5, clip_value=1.0,
                 engine=None, optimizer="adam", momentum=0.9, lr_decay=0.0):
        if model.wide:
            raise NotImplementedError("the fused fine-tuning step runs the 64-channel kernels; wider models take the API path")
        self.model, self.head = model, head
        self.dev = next(model.parameters()).device
        self.flat, self.n_live = flatten_parameters(model)
        self.live = self.flat[: self.n_live]
        self.flat_grad, self.grad_views = flat_grad_views(model, self.n_live, self.dev)
        self.hflat, self.hgrad, self.dW, self.db = flatten_head(head)
        self.gin = model.engine()
        self.eng = engine if engine is not None else ClsHeadEngine()
        if optimizer == "adam":
            self.optimizer = FlatAdamClipValue(self.live, self.flat_grad, learning_rate, betas, weight_decay, clip_value, self.eng)
        elif optimizer == "sgd":
            self.optimizer = FlatSGDClipValue(self.live, self.flat_grad, learning_rate, momentum, weight_decay, clip_value, self.eng)
        elif optimizer == "adagrad":
            self.optimizer = FlatAdagradClipValue(self.live, self.flat_grad, learning_rate, lr_decay, weight_decay, clip_value, self.eng)
        else:
            raise ValueError(f"unknown optimizer {optimizer!r} (adam, sgd, adagrad)")
        self.head_optimizer = FlatAdamClipValue(self.hflat, self.hgrad, learning_rate, betas, weight_decay, clip_value, self.eng)
        self.mask_fn = None          # tests inject explicit dropout keep-masks [L + 1, B, 64] here; default = in-kernel Philox
        self.dropout_seed = 0x5EED1000
        self.meter_acc, self.meter_max = _meter_buffers(self.dev)
        self._dfeat = {}
        self.last = None

    def step(self, step, graph_q, labels, lr):
        """one training step on the current stream; -> dict(loss, correct, logits, dlogits, feat) (device tensors)"""
        st = _cabi.raw_stream(self.dev)
        model = self.model
        model.train()
        B = graph_q.batch_size
        keep = self.mask_fn() if self.mask_fn is not None else None
        seed = (self.dropout_seed + step * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF if model.gnn.drop.p > 0 else None
        p, buf = self.gin.make_pass(model, graph_q, training=True, keep=keep, slot=("finetune", 0), dropout_seed=seed)
        self.gin.forward([p], stream=st)                                            # feat_q = model(graph_q)
        feat = buf["feat"]
        D = model.output_dim
        if B not in self._dfeat:
            self._dfeat[B] = torch.zeros(B, H, dtype=torch.float32, device=self.dev)
        dfeat = self._dfeat[B]
        W, b = self.head.weight, self.head.bias
        out = self.eng.train(feat, W, b, labels, self.dW, self.db, dfeat, meters=(self.meter_acc, self.meter_max, graph_q),
                             stream=st)                                             # out, loss, loss.backward() of the head
        assert W.shape[1] == D
        self.gin.backward(model, p, buf, dfeat, targets=self.grad_views, stream=st)   # loss.backward() of the encoder
        for opt in (self.optimizer, self.head_optimizer):                             # :237-243: the same lr for both
            opt.param_groups[0]["lr"] = lr
        self.optimizer.step(stream=st)                                              # clip_grad_value_ + optimizer.step()
        self.head_optimizer.step(stream=st)                                         # ... + output_layer_optimizer.step()
        out["feat"] = feat
        self.last = (p, buf)
        return out

    def read_meters(self):
        """-> (acc list[5], mx list[2]) and zeroes them; synchronises (once per log line)"""
        a, m = self.meter_acc.tolist(), self.meter_max.tolist()
        self.meter_acc.zero_()
        self.meter_max.zero_()
        return a, m


class LabeledProducer:
    """Makes the next labelled batch on a side stream while the current step runs -- the role of the reference's DataLoader
    workers.  The dataset's sampler / positional-embedding rings must hold ``depth + 2`` batches: a slot is rewritten only
    after the step that consumed it has been issued and an event recorded behind it."""

    def __init__(self, dataset, device, prefetch=True, depth=1):
        self.ds, self.dev = dataset, torch.device(device)
        self.prefetch = bool(prefetch) and self.dev.type == "cuda"
        self.depth = depth
        self.side = torch.cuda.Stream(self.dev) if self.prefetch else None
        self._released = []

    def __iter__(self):
        raise TypeError("use batches(order)")

    def batches(self, order):
        order = np.asarray(order, dtype=np.int64)
        B = self.ds.batch_size
        chunks = [order[lo:lo + B] for lo in range(0, len(order), B)]
        # a dataset that can upload the epoch's order once hands out one call per batch (GraphClassificationDatasetLabeled)
        calls = self.ds.batch_calls(order) if hasattr(self.ds, "batch_calls") else [
            (lambda c=c: self.ds.make_batch(c)) for c in chunks]
        if not self.prefetch:
            for call in calls:
                yield call()
            return
        pending = []
        main = torch.cuda.current_stream(self.dev)

        def launch(i):
            with torch.cuda.stream(self.side):
                self.side.wait_stream(main) if not self._released else self.side.wait_event(self._released[0])
                q, lab = calls[i]()
                ev = torch.cuda.Event()
                ev.record(self.side)
            pending.append((q, lab, ev))

        nxt = 0
        for i in range(len(chunks)):
            while nxt < len(chunks) and nxt <= i + self.depth:
                launch(nxt)
                nxt += 1
            q, lab, ev = pending.pop(0)
            main.wait_event(ev)
            yield q, lab
            done = torch.cuda.Event()
            done.record(main)                              # the step that consumed this batch has been issued before it
            self._released.append(done)
            if len(self._released) > 1:
                self._released.pop(0)


def evaluate(model, head, dataset, order, engine=None, stream=None):
    """test_finetune (train.py:300-337 of the reference): eval mode, the fused eval encoder on the q view plus the head's
    eval call per batch; loss and F1 accumulate on the device and are read once.  -> (loss, f1) averaged over the rows (the
    reference weights each batch's mean by its size)."""
    eng = engine if engine is not None else ClsHeadEngine()
    dev = next(model.parameters()).device
    model.eval()
    loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    W, b = head.weight.detach(), head.bias.detach()
    st = _cabi.raw_stream(dev)
    for graph_q, labels in dataset.batches(order):
        feat = embed_eval(model, graph_q, st)
        eng.eval(feat, W.contiguous(), b.contiguous(), labels, loss_sum, counts, stream=st)
    n = max(int(counts[1].item()), 1)
    return float(loss_sum.item()) / n, int(counts[0].item()) / n


def embed_eval(model, graph_q, st=None):
    """model(graph_q) in eval mode: one gcc_gin_eval_fused launch (fused 64-channel kernels) -> [B, 64] device tensor
    (columns past output_dim zero); wide and GAT models through GraphEncoder.forward"""
    if model.wide or model.gnn_model == "gat":
        with torch.no_grad():
            return model(graph_q).contiguous()
    eng = model.engine()
    p, buf = eng.make_pass(model, graph_q, training=False, slot=("finetune", "eval"))
    eng.eval_fused([p], stream=st)
    return buf["feat"]


class _ClsHeadFn(torch.autograd.Function):
    """output_layer(feat) + CrossEntropyLoss through autograd, on the HIP head (the API path: SGD / Adagrad, wide models)"""

    @staticmethod
    def forward(ctx, feat, W, b, labels, engine):
        feat = feat.contiguous()
        dW, db = torch.empty_like(W), torch.empty_like(b)
        dfeat = torch.empty_like(feat)
        st = _cabi.raw_stream(feat)
        out = engine.train(feat, W.detach().contiguous(), b.detach().contiguous(), labels, dW, db, dfeat, stream=st)
        ctx.save_for_backward(dW, db, dfeat)
        ctx.mark_non_differentiable(out["logits"], out["correct"])
        return out["loss"].reshape(()), out["logits"], out["correct"]

    @staticmethod
    def backward(ctx, dloss, _dlogits, _dcorrect):
        dW, db, dfeat = ctx.saved_tensors
        return dfeat * dloss, dW * dloss, db * dloss, None, None


def cls_head_loss(feat, head: nn.Linear, labels, engine=None):
    """-> (loss, logits, correct int32[2]) with loss differentiable w.r.t. feat and the head's parameters"""
    return _ClsHeadFn.apply(feat, head.weight, head.bias, labels, engine or ClsHeadEngine())
