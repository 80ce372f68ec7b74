"""``main`` of the reference's train.py for ``--finetune`` (train.py:480-797): resume override, labelled dataset, stratified fold,
head + two optimizers, epochs of train_finetune, checkpoints, and test_finetune after the last epoch.  Returns the held-out
F1 (``--cv`` collects ten of them, train.py:800-815)."""
from __future__ import annotations

import os
import time

import numpy as np
import psutil
import torch
import torch.nn as nn

from .misc import AverageMeter, adjust_learning_rate, warmup_linear

GRAPH_CLASSIFICATION_DSETS = ["collab", "imdb-binary", "imdb-multi", "rdt-b", "rdt-5k"]


def fold_split(labels, fold_idx, seed):
    """train.py:531-543: StratifiedKFold(n_splits=10, shuffle=True, random_state=seed) -> (train_idx, test_idx)"""
    try:
        from sklearn.model_selection import StratifiedKFold
    except ImportError as e:                    # never another split silently: the folds are the reference's or none
        raise RuntimeError("--finetune needs scikit-learn (the reference's StratifiedKFold picks the folds)") from e
    assert 0 <= fold_idx < 10, "fold_idx must be from 0 to 9."
    skf = StratifiedKFold(n_splits=10, shuffle=True, random_state=seed)
    idx_list = list(skf.split(np.zeros(len(labels)), labels))
    return idx_list[fold_idx]


def apply_resume(args, checkpoint_opt):
    """train.py:487-505: the checkpoint's options, with these of the command line"""
    pretrain_args = checkpoint_opt
    for name in ("fold_idx", "gpu", "finetune", "resume", "cv", "dataset", "epochs", "num_workers", "batch_size",
                 "edgelist", "nodelabel", "tudataset", "graphs_npz", "edge_multiplicity", "no_prefetch", "graph_batcher", "tu_parse",
                 "step_path"):
        setattr(pretrain_args, name, getattr(args, name, None))
    if args.dataset in GRAPH_CLASSIFICATION_DSETS:
        pretrain_args.num_workers = 0           # train.py:500-502
    return pretrain_args


def load_labelled(args, device):
    """-> dataset (gcc_amd.datasets.*Labeled) from --edgelist/--nodelabel, --tudataset or --graphs-npz"""
    from . import ingest
    from .datasets import GraphClassificationDatasetLabeled, NodeClassificationDatasetLabeled

    kw = dict(dataset=args.dataset, rw_hops=args.rw_hops, subgraph_size=args.subgraph_size, restart_prob=args.restart_prob,
              positional_embedding_size=args.positional_embedding_size, batch_size=args.batch_size, device=device)
    mult = getattr(args, "edge_multiplicity", 0) or 0
    if args.dataset in GRAPH_CLASSIFICATION_DSETS:
        tu_parse = getattr(args, "tu_parse", None) or "host"
        batcher = getattr(args, "graph_batcher", None) or "auto"
        if tu_parse not in ("host", "device"):
            raise SystemExit(f"--tu-parse {tu_parse!r}: host or device")
        if tu_parse == "device":
            if not getattr(args, "tudataset", None):
                raise SystemExit("--tu-parse device says where the files of --tudataset are parsed: pass --tudataset")
            if batcher == "host":
                raise SystemExit("--tu-parse device builds the resident corpus of the device batcher: not with --graph-batcher host")
            from .tu_ingest import TUIngestEngine

            d = TUIngestEngine(device=device).read_tudataset(args.tudataset, args.dataset)
            return GraphClassificationDatasetLabeled(corpus=d["corpus"], labels=d["graph_labels"], edge_multiplicity=max(mult, 1),
                                                     run_seed=args.seed, batcher=batcher, **kw)
        if getattr(args, "tudataset", None):
            d = ingest.read_tudataset(args.tudataset, args.dataset)
            graphs, labels = d["graphs"], d["graph_labels"]
        elif getattr(args, "graphs_npz", None):
            z = np.load(args.graphs_npz)
            no, rp, ci = z["node_off"].astype(np.int64), z["row_ptr"].astype(np.int64), z["col_idx"].astype(np.int64)
            graphs = [(rp[no[i]:no[i + 1] + 1] - rp[no[i]], ci[rp[no[i]]:rp[no[i + 1]]]) for i in range(len(no) - 1)]
            labels = z["graph_labels"].astype(np.int64)
        else:
            raise SystemExit(f"--finetune on {args.dataset} (graph classification) needs --tudataset <folder> or --graphs-npz "
                             "(dataset files are not bundled)")
        return GraphClassificationDatasetLabeled(graphs=graphs, labels=labels, edge_multiplicity=max(mult, 1),
                                                 run_seed=args.seed, batcher=getattr(args, "graph_batcher", None) or "auto",
                                                 **kw)
    if not getattr(args, "edgelist", None) or not getattr(args, "nodelabel", None):
        raise SystemExit(f"--finetune on {args.dataset} (node classification) needs --edgelist data/<name>/<name>.edgelist and "
                         "--nodelabel data/<name>/<name>.nodelabel (dataset files are not bundled)")
    d = ingest.read_edgelist(args.edgelist, args.nodelabel, hindex="hindex" in args.dataset)        # (as generate.py reads it)
    return NodeClassificationDatasetLabeled(graph=(d["row_ptr"], d["col_idx"]), labels=d["y"],
                                            edge_multiplicity=mult or d["edge_multiplicity"], run_seed=args.seed,
                                            num_buffers=3, **kw)


class _NullWriter:
    def add_scalar(self, *a, **k):
        pass


def _summary_writer(folder):
    try:
        from torch.utils.tensorboard import SummaryWriter

        return SummaryWriter(folder)
    except Exception:
        return _NullWriter()


def main_finetune(args, option_update):
    from .encoder import encoder_from_opt
    from .finetune import FinetuneTrainStep, LabeledProducer, clear_bn, cls_head_loss, evaluate
    from .train_step import flatten_parameters, resolve_step_path

    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("--finetune runs on one GPU (the reference's fine-tuning is single-GPU)")
    args.step_path = step_path = getattr(args, "step_path", "auto")
    if not args.resume:                                             # refusals before any device work
        resolve_step_path(step_path, optimizer=args.optimizer, gat=args.model == "gat", wide=args.hidden_size > 64, moco=False,
                          finetune=True)
    np.random.seed(args.seed)                                       # train.py:482-485
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    checkpoint = None
    if args.resume:
        if os.path.isfile(args.resume):
            print("=> loading checkpoint '{}'".format(args.resume))
            checkpoint = torch.load(args.resume, map_location="cpu", weights_only=False)
            args = apply_resume(args, checkpoint["opt"])
        else:
            print("=> no checkpoint found at '{}'".format(args.resume))
    args = option_update(args)
    print(args)
    assert args.gpu is not None and torch.cuda.is_available()
    print("Use GPU: {} for training".format(args.gpu))
    assert args.positional_embedding_size % 2 == 0
    torch.cuda.set_device(args.gpu)
    dev = torch.device("cuda", args.gpu)

    dataset = load_labelled(args, dev)                              # train.py:516-545
    train_idx, test_idx = fold_split(dataset.labels.tolist(), args.fold_idx, args.seed)

    model = encoder_from_opt(args).to(dev)                          # train.py:601-620
    from .contrast import MemoryMoCo

    contrast = MemoryMoCo(args.hidden_size, None, args.nce_k, args.nce_t, use_softmax=True).to(dev)   # (checkpointed only)
    output_layer = nn.Linear(in_features=args.hidden_size, out_features=dataset.num_classes).to(dev)  # train.py:637-646
    fused = resolve_step_path(step_path, optimizer=args.optimizer, gat=model.gnn_model != "gin", wide=model.wide, moco=False,
                              finetune=True) == "fused"
    if fused:
        flatten_parameters(model)
    clear_bn(model)                                                 # train.py:651-655 (before the resume, as there)
    args.start_epoch = 1
    if checkpoint is not None:                                      # train.py:685-702: in place, into the flat buffers
        model.load_state_dict(checkpoint["model"])
        contrast.load_state_dict(checkpoint["contrast"])
        print("=> loaded successfully '{}' (epoch {})".format(args.resume, checkpoint["epoch"]))
        del checkpoint
        torch.cuda.empty_cache()
    if fused:
        trainer = FinetuneTrainStep(model, output_layer, learning_rate=args.learning_rate, betas=(args.beta1, args.beta2),
                                    weight_decay=args.weight_decay, clip_value=1.0, optimizer=args.optimizer,
                                    momentum=args.momentum, lr_decay=args.lr_decay_rate)
        optimizer, head_optimizer = trainer.optimizer, trainer.head_optimizer
    else:                                                           # API path: wide and GAT models, SGD / Adagrad by default (train.py:658-679)
        trainer = None
        head_optimizer = torch.optim.Adam(output_layer.parameters(), lr=args.learning_rate, betas=(args.beta1, args.beta2),
                                          weight_decay=args.weight_decay)
        if args.optimizer == "sgd":
            optimizer = torch.optim.SGD(model.parameters(), lr=args.learning_rate, momentum=args.momentum,
                                        weight_decay=args.weight_decay)
        elif args.optimizer == "adam":
            optimizer = torch.optim.Adam(model.parameters(), lr=args.learning_rate, betas=(args.beta1, args.beta2),
                                         weight_decay=args.weight_decay)
        else:
            optimizer = torch.optim.Adagrad(model.parameters(), lr=args.learning_rate, lr_decay=args.lr_decay_rate,
                                            weight_decay=args.weight_decay)
    producer = LabeledProducer(dataset, dev, prefetch=not getattr(args, "no_prefetch", False))
    gen = torch.Generator().manual_seed(args.seed)                  # the train loader's shuffle (train.py:575-583)
    sw = _summary_writer(args.tb_folder)
    n_batch = (len(train_idx) + args.batch_size - 1) // args.batch_size       # no drop_last: the last batch is partial
    for epoch in range(args.start_epoch, args.epochs + 1):
        adjust_learning_rate(epoch, args, optimizer)
        print("==> training...")
        time1 = time.time()
        order = train_idx[torch.randperm(len(train_idx), generator=gen).numpy()]
        train_finetune(epoch, producer.batches(order), n_batch, model, output_layer, trainer, optimizer, head_optimizer,
                       sw, args, cls_head_loss)
        torch.cuda.synchronize()
        print("epoch {}, total time {:.2f}".format(epoch, time.time() - time1))
        dataset.check_status()
        state = {"opt": args, "model": model.state_dict(), "contrast": contrast.state_dict(),       # train.py:747-786
                 "optimizer": optimizer.state_dict(), "epoch": epoch}
        if epoch % args.save_freq == 0:
            print("==> Saving...")
            torch.save(state, os.path.join(args.model_folder, "ckpt_epoch_{epoch}.pth".format(epoch=epoch)))
        print("==> Saving...")
        torch.save(state, os.path.join(args.model_folder, "current.pth"))
        del state
    valid_loss, valid_f1 = evaluate(model, output_layer, dataset, test_idx)                         # train.py:788-791
    global_step = (epoch + 1) * n_batch
    sw.add_scalar("ft_loss/valid", valid_loss, global_step)
    sw.add_scalar("ft_f1/valid", valid_f1, global_step)
    print(f"Epoch {epoch}, loss {valid_loss:.3f}, f1 {valid_f1:.3f}")
    return valid_f1


def train_finetune(epoch, batches, n_batch, model, output_layer, trainer, optimizer, head_optimizer, sw, opt, cls_head_loss):
    """train.py:175-297 of the reference; the meters are accumulated on the device and read once per log line"""
    batch_time, data_time = AverageMeter(), AverageMeter()
    loss_meter, f1_meter, graph_size = AverageMeter(), AverageMeter(), AverageMeter()
    epoch_loss_meter, epoch_f1_meter = AverageMeter(), AverageMeter()
    max_num_nodes = max_num_edges = 0
    dev = next(model.parameters()).device
    acc = torch.zeros(5, dtype=torch.float64, device=dev)
    mx = torch.zeros(2, dtype=torch.int32, device=dev)
    end = time.time()
    for idx, (graph_q, y) in enumerate(batches):
        data_time.update(time.time() - end)
        global_step = epoch * n_batch + idx
        lr_this_step = opt.learning_rate * warmup_linear(global_step / (opt.epochs * n_batch), 0.1)
        if trainer is not None:
            trainer.step(global_step, graph_q, y, lr_this_step)
        else:
            model.train()
            output_layer.train()
            feat_q = model(graph_q)
            loss, _out, correct = cls_head_loss(feat_q, output_layer, y)
            optimizer.zero_grad()
            head_optimizer.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_value_(model.parameters(), 1)
            torch.nn.utils.clip_grad_value_(output_layer.parameters(), 1)
            for o in (optimizer, head_optimizer):
                for pg in o.param_groups:
                    pg["lr"] = lr_this_step
            optimizer.step()
            head_optimizer.step()
            B = graph_q.batch_size
            v = correct[1].double()
            acc += torch.stack([loss.detach().double() * v, correct[0].double(), v,
                                graph_q.node_off[B].double(), torch.ones((), dtype=torch.float64, device=dev)])
            mx.copy_(torch.maximum(mx, torch.stack([graph_q.node_off[B], graph_q.edge_off[B]])))
        last = idx + 1 == n_batch
        if (idx + 1) % opt.print_freq == 0 or (idx + 1) % opt.tb_freq == 0 or last:
            if trainer is not None:
                a, m = trainer.read_meters()
            else:
                a, m = acc.tolist(), mx.tolist()
                acc.zero_()
                mx.zero_()
            rows = max(a[2], 1.0)
            loss_meter.update(a[0] / rows, rows)
            epoch_loss_meter.update(a[0] / rows, rows)
            f1_meter.update(a[1] / rows, rows)
            epoch_f1_meter.update(a[1] / rows, rows)
            graph_size.update(a[3] / rows, rows)
            max_num_nodes, max_num_edges = max(max_num_nodes, m[0]), max(max_num_edges, m[1])
        batch_time.update(time.time() - end)
        end = time.time()
        if (idx + 1) % opt.print_freq == 0:
            mem = psutil.virtual_memory()
            print("Train: [{0}][{1}/{2}]\t"
                  "BT {batch_time.val:.3f} ({batch_time.avg:.3f})\t"
                  "DT {data_time.val:.3f} ({data_time.avg:.3f})\t"
                  "loss {loss.val:.3f} ({loss.avg:.3f})\t"
                  "f1 {f1.val:.3f} ({f1.avg:.3f})\t"
                  "GS {graph_size.val:.3f} ({graph_size.avg:.3f})\t"
                  "mem {mem:.3f}".format(epoch, idx + 1, n_batch, batch_time=batch_time, data_time=data_time,
                                         loss=loss_meter, f1=f1_meter, graph_size=graph_size, mem=mem.used / 1024 ** 3))
        if (idx + 1) % opt.tb_freq == 0:
            sw.add_scalar("ft_loss", loss_meter.avg, global_step)
            sw.add_scalar("ft_f1", f1_meter.avg, global_step)
            sw.add_scalar("graph_size", graph_size.avg, global_step)
            sw.add_scalar("lr", lr_this_step, global_step)
            sw.add_scalar("graph_size/max", max_num_nodes, global_step)
            sw.add_scalar("graph_size/max_edges", max_num_edges, global_step)
            loss_meter.reset()
            f1_meter.reset()
            graph_size.reset()
            max_num_nodes, max_num_edges = 0, 0
    return epoch_loss_meter.avg, epoch_f1_meter.avg
