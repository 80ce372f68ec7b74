#!/usr/bin/env python
"""Drop-in for the reference's generate.py (node-classification datasets): load a pre-trained checkpoint, embed every
node of a graph as (f(q) + f(k)) / 2 over its two RWR views with the eval-mode encoder, save
``<model_folder>/<dataset>.npy`` (generate.py:56-125).  The graph comes from ``--edgelist`` (the reference's
``data/<name>/<name>.edgelist`` format, gcc/datasets/data_util.py:61-110) or ``--graph-npz`` (row_ptr/col_idx);
everything runs on the GPU (sampler, positional embedding, encoder).

Extra flags (not in the reference): --edgelist / --nodelabel / --graph-npz / --graphs-npz / --tudataset / --edge-multiplicity /
--batch-size / --wide-eval / --graph-batcher.  ``--wide-eval resident`` embeds with a wide GIN checkpoint (--hidden-size above 64, f32- or
bf16-trained) through one gcc_ginw_embed call per batch: bf16 layers resident in LDS, f32 readout (DESIGN.md section 7b has
the rounding rule the flag opts into); the default, ``chain``, is the any-width eval chain.  Graph-classification datasets (entire_graph=True, generate.py:75-82) come as ``--graphs-npz``: node_off
[G+1], row_ptr [N+1] (per-graph offsets restarting at 0 are rebuilt from node_off), col_idx (local ids)."""
import argparse
import os

import numpy as np
import torch


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
        from gcc_amd.datasets import NodeClassificationDataset

        ds = NodeClassificationDataset(device=self.device, **kw)
        return ds, ds.sampler.node_cap, ds.sampler.check_status

    def posemb(self, batch_size, node_cap, size, seed):
        from gcc_amd.posemb import DevicePosEmb

        return DevicePosEmb(batch_size, node_cap, size, device=self.device, seed=seed, max_views=2, num_buffers=2)

    def place(self, model):
        return model.to(self.device)


def main(args_test, pipeline=None):
    from gcc_amd import ingest
    from gcc_amd.datasets import GraphClassificationDataset
    from gcc_amd.encoder import encoder_from_opt
    from gcc_amd.generate import test_moco

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
    if args_test.tudataset:
        graphs = ingest.read_tudataset(args_test.tudataset, args_test.dataset)["graphs"]
        graph, mult = None, max(args_test.edge_multiplicity, 1)
    elif args_test.graphs_npz:
        z = np.load(args_test.graphs_npz)
        no, rp, ci = z["node_off"].astype(np.int64), z["row_ptr"].astype(np.int64), z["col_idx"].astype(np.int64)
        graphs = [(rp[no[i]:no[i + 1] + 1] - rp[no[i]], ci[rp[no[i]]:rp[no[i + 1]]]) for i in range(len(no) - 1)]
        graph, mult = None, max(args_test.edge_multiplicity, 1)
    elif args_test.edgelist:
        d = ingest.read_edgelist(args_test.edgelist, args_test.nodelabel, hindex="hindex" in args_test.dataset)
        graph, mult = (d["row_ptr"], d["col_idx"]), d["edge_multiplicity"]
    elif args_test.graph_npz:
        z = np.load(args_test.graph_npz)
        graph, mult = (z["row_ptr"], z["col_idx"]), args_test.edge_multiplicity
    else:
        raise SystemExit("pass --edgelist data/<name>/<name>.edgelist, --graph-npz, --graphs-npz or --tudataset (dataset files are not bundled)")
    if args_test.edge_multiplicity:
        mult = args_test.edge_multiplicity
    if graphs is not None:
        train_dataset = GraphClassificationDataset(                  # generate.py:75-82
            dataset=args_test.dataset, rw_hops=args.rw_hops, subgraph_size=args.subgraph_size,
            restart_prob=args.restart_prob, positional_embedding_size=args.positional_embedding_size,
            graphs=graphs, edge_multiplicity=mult, batch_size=args_test.batch_size, device=args.device,
            batcher=getattr(args_test, "graph_batcher", None) or "auto")
        node_cap = train_dataset.node_cap
    else:
        train_dataset, node_cap, check_sampler = pipeline.node_dataset(      # generate.py:84-91
            dataset=args_test.dataset, rw_hops=args.rw_hops, subgraph_size=args.subgraph_size,
            restart_prob=args.restart_prob, positional_embedding_size=args.positional_embedding_size,
            graph=graph, edge_multiplicity=mult, batch_size=args_test.batch_size, run_seed=getattr(args, "seed", 0))
    model = pipeline.place(model)
    model.load_state_dict(checkpoint["model"])
    del checkpoint
    posemb = pipeline.posemb(args_test.batch_size, node_cap, args.positional_embedding_size, getattr(args, "seed", 0))
    emb = test_moco(train_dataset, model, posemb, args)
    if graphs is None:
        check_sampler()
    else:
        train_dataset.check_status()
    posemb.check_status()
    if model.resident_eval:
        model.resident_engine().check_status()                       # (before anything is written)
    os.makedirs(args.model_folder, exist_ok=True)
    out = os.path.join(args.model_folder, args_test.dataset)
    np.save(out, emb.numpy())
    print("saved {}.npy {}".format(out, tuple(emb.shape)))


if __name__ == "__main__":
    parser = argparse.ArgumentParser("argument for training")
    # fmt: off
    parser.add_argument("--load-path", type=str, help="path to load model")
    parser.add_argument("--dataset", type=str, default="dgl")
    parser.add_argument("--gpu", default=None, type=int, help="GPU id to use.")
    # ---- not in the reference: where the graph comes from
    parser.add_argument("--edgelist", type=str, default=None, help="<name>.edgelist of the reference's data folder")
    parser.add_argument("--nodelabel", type=str, default=None, help="<name>.nodelabel (only read to validate the node set)")
    parser.add_argument("--graph-npz", type=str, default=None, help="npz with row_ptr/col_idx of the simple symmetric graph")
    parser.add_argument("--graphs-npz", type=str, default=None, help="npz with node_off/row_ptr/col_idx of a list of small graphs (graph classification)")
    parser.add_argument("--tudataset", type=str, default=None, help="folder with the raw TU files <NAME>_A.txt, <NAME>_graph_indicator.txt, <NAME>_graph_labels.txt of --dataset (imdb-binary, imdb-multi, rdt-b, rdt-5k, collab)")
    parser.add_argument("--edge-multiplicity", type=int, default=0, help="copies of every edge in the reference's DGL graph (edge lists: detected; npz: default 2)")
    parser.add_argument("--batch-size", type=int, default=256)
    parser.add_argument("--graph-batcher", choices=["auto", "host", "device"], default="auto", help="--graphs-npz / --tudataset: assemble batches on the device (gcc_pack_graphs; auto on a GPU) or with the host loop")
    parser.add_argument("--wide-eval", choices=["chain", "resident"], default="chain", help="wide GIN checkpoints: the any-width eval chain (f32 or the checkpoint's --encoder-dtype), or one LDS-resident bf16 call per batch (gcc_ginw_embed; f32 readout)")
    # fmt: on
    a = parser.parse_args()
    if a.graph_npz and not a.edge_multiplicity:
        a.edge_multiplicity = 2
    main(a)
