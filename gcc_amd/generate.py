"""``test_moco`` of the reference's generate.py:33-53 -- eval-mode encoder over every node's two views, embedding =
(f(q) + f(k)) / 2 -- on the device pipeline, and the
body of the generate.py command (``run``), which the similarity-search task also calls to embed its two networks."""
from __future__ import annotations

import os

import numpy as np
import torch


def test_moco(dataset, model, posemb, opt=None):
    """dataset: gcc_amd.datasets.NodeClassificationDataset; model: gcc_amd.encoder.GraphEncoder;
    posemb: gcc_amd.posemb.DevicePosEmb (max_views >= 2).  Returns a CPU tensor [len(dataset), hidden]."""
    model.eval()                                                   # generate.py:38
    emb_list = []
    for graph_q, graph_k in dataset:
        bsz = graph_q.batch_size
        views = [graph_q] if graph_k is graph_q else [graph_q, graph_k]       # entire_graph: both views are one graph
        posemb.multi(views) if hasattr(posemb, "multi") else [posemb(v) for v in views]
        with torch.no_grad():
            if getattr(model, "fused_eval", False):
                # both views through the encoder AND (feat_q + feat_k) / 2 in one launch (gcc_gin_eval_fused)
                emb = model.embed_views(graph_q, graph_k)
            else:
                feat_q = model(graph_q)
                feat_k = feat_q if graph_k is graph_q else model(graph_k)
                emb = (feat_q + feat_k) / 2
        if opt is not None:
            assert emb.shape == (bsz, opt.hidden_size)             # generate.py:51
        emb_list.append(emb[: graph_q.valid].detach().cpu())
    return torch.cat(emb_list)


class DevicePipeline:
    """Where the sampler, the positional embedding and the encoder run: the GPU.  The emulator tests pass main() an object
    with the same four members (device, node_dataset, posemb, place) that builds them on the emulator library instead."""

    def __init__(self, gpu):
        assert torch.cuda.is_available(), "the device pipeline needs a GPU"
        self.gpu = 0 if gpu is None else gpu
        print("Use GPU: {} for generation".format(self.gpu))
        self.device = torch.device("cuda", self.gpu)
        torch.cuda.set_device(self.device)

    def node_dataset(self, **kw):
        """-> (NodeClassificationDataset on the device sampler, its node capacity, its status check)"""
        from .datasets import NodeClassificationDataset

        ds = NodeClassificationDataset(device=self.device, **kw)
        return ds, ds.sampler.node_cap, ds.sampler.check_status

    def posemb(self, batch_size, node_cap, size, seed):
        from .posemb import DevicePosEmb

        return DevicePosEmb(batch_size, node_cap, size, device=self.device, seed=seed, max_views=2, num_buffers=2)

    def place(self, model):
        return model.to(self.device)


def run(args_test, pipeline=None, save=True):
    """generate.py's main (generate.py:56-125 of the reference): checkpoint + graph source of ``args_test`` -> the embedding
    table (CPU tensor), saved as ``<model_folder>/<dataset>.npy`` unless ``save`` is False.  ``pipeline``: where the sampler,
    the positional embedding and the encoder run (default: DevicePipeline)."""
    from . import ingest
    from .datasets import GraphClassificationDataset
    from .encoder import encoder_from_opt

    if os.path.isfile(args_test.load_path):
        print("=> loading checkpoint '{}'".format(args_test.load_path))
        checkpoint = torch.load(args_test.load_path, map_location="cpu", weights_only=False)
        print("=> loaded successfully '{}' (epoch {})".format(args_test.load_path, checkpoint["epoch"]))
    else:
        raise SystemExit("=> no checkpoint found at '{}'".format(args_test.load_path))
    args = checkpoint["opt"]
    if pipeline is None:
        pipeline = DevicePipeline(args_test.gpu)
        args.gpu = pipeline.gpu
    args.device = pipeline.device
    model = encoder_from_opt(args)                                   # generate.py:102-118
    if getattr(args_test, "wide_eval", "chain") == "resident":       # (refused before anything is read or built)
        if getattr(model, "gnn_model", None) != "gin" or not model.wide:
            raise SystemExit("--wide-eval resident serves wide GIN checkpoints (--model gin with --hidden-size above 64); this one is "
                             "--model {} --hidden-size {}: drop the flag".format(args.model, args.hidden_size))
        model.resident_eval = True

    graphs = None
    multigraph = False
    tu_corpus = None
    tu_parse = getattr(args_test, "tu_parse", None) or "host"
    if tu_parse not in ("host", "device"):
        raise SystemExit(f"--tu-parse {tu_parse!r}: host or device")
    if tu_parse == "device":
        if not args_test.tudataset:
            raise SystemExit("--tu-parse device says where the files of --tudataset are parsed: pass --tudataset")
        if (getattr(args_test, "graph_batcher", None) or "auto") == "host":
            raise SystemExit("--tu-parse device builds the resident corpus of the device batcher: not with --graph-batcher host")
        from .tu_ingest import TUIngestEngine

        tu_corpus = TUIngestEngine(device=args.device).read_tudataset(args_test.tudataset, args_test.dataset)["corpus"]
        graph, mult = None, max(args_test.edge_multiplicity, 1)
    elif args_test.tudataset:
        graphs = ingest.read_tudataset(args_test.tudataset, args_test.dataset)["graphs"]
        graph, mult = None, max(args_test.edge_multiplicity, 1)
    elif args_test.graphs_npz:
        z = np.load(args_test.graphs_npz)
        no, rp, ci = z["node_off"].astype(np.int64), z["row_ptr"].astype(np.int64), z["col_idx"].astype(np.int64)
        graphs = [(rp[no[i]:no[i + 1] + 1] - rp[no[i]], ci[rp[no[i]]:rp[no[i + 1]]]) for i in range(len(no) - 1)]
        graph, mult = None, max(args_test.edge_multiplicity, 1)
    elif args_test.edgelist:
        # pairs listed a non-uniform number of times become parallel edges: repeated entries of the CSR rows
        d = ingest.read_edgelist(args_test.edgelist, args_test.nodelabel, hindex="hindex" in args_test.dataset, multigraph=True)
        graph, mult, multigraph = (d["row_ptr"], d["col_idx"]), d["edge_multiplicity"], d["multigraph"]
    elif getattr(args_test, "ss_graph", None):
        # a weighted co-author network of the similarity-search task (data/panther/<name>.graph + .dict): weight t = t
        # parallel edges; one row of the output per node of the graph file, in the reader's index order
        dict_path = getattr(args_test, "ss_dict", None) or os.path.splitext(args_test.ss_graph)[0] + ".dict"
        d = ingest.read_ss_graph(args_test.ss_graph, dict_path, csr=True)
        graph, mult, multigraph = (d["row_ptr"], d["col_idx"]), d["edge_multiplicity"], True
    elif args_test.graph_npz:
        z = np.load(args_test.graph_npz)
        graph, mult = (z["row_ptr"], z["col_idx"]), args_test.edge_multiplicity
    else:
        raise SystemExit("pass --edgelist data/<name>/<name>.edgelist, --ss-graph data/panther/<name>.graph, --graph-npz, --graphs-npz or --tudataset (dataset files are not bundled)")
    if args_test.edge_multiplicity:
        mult = args_test.edge_multiplicity
    if graphs is not None or tu_corpus is not None:
        train_dataset = GraphClassificationDataset(                  # generate.py:75-82
            dataset=args_test.dataset, rw_hops=args.rw_hops, subgraph_size=args.subgraph_size,
            restart_prob=args.restart_prob, positional_embedding_size=args.positional_embedding_size,
            graphs=graphs, corpus=tu_corpus, edge_multiplicity=mult, batch_size=args_test.batch_size, device=args.device,
            batcher=getattr(args_test, "graph_batcher", None) or "auto")
        node_cap = train_dataset.node_cap
    else:
        train_dataset, node_cap, check_sampler = pipeline.node_dataset(      # generate.py:84-91
            dataset=args_test.dataset, rw_hops=args.rw_hops, subgraph_size=args.subgraph_size,
            restart_prob=args.restart_prob, positional_embedding_size=args.positional_embedding_size,
            graph=graph, edge_multiplicity=mult, batch_size=args_test.batch_size, run_seed=getattr(args, "seed", 0),
            **({"multigraph": True} if multigraph else {}))
    model = pipeline.place(model)
    model.load_state_dict(checkpoint["model"])
    del checkpoint
    posemb = pipeline.posemb(args_test.batch_size, node_cap, args.positional_embedding_size, getattr(args, "seed", 0))
    emb = test_moco(train_dataset, model, posemb, args)
    if graphs is None and tu_corpus is None:
        check_sampler()
    else:
        train_dataset.check_status()
    posemb.check_status()
    if model.resident_eval:
        model.resident_engine().check_status()                       # (before anything is written)
    if save:
        os.makedirs(args.model_folder, exist_ok=True)
        out = os.path.join(args.model_folder, args_test.dataset)
        np.save(out, emb.numpy())
        print("saved {}.npy {}".format(out, tuple(emb.shape)))
    return emb
