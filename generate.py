#!/usr/bin/env python
"""Drop-in for the reference's generate.py (node-classification datasets): load a pre-trained checkpoint, embed every
node of a graph as (f(q) + f(k)) / 2 over its two RWR views with the eval-mode encoder, save
``<model_folder>/<dataset>.npy`` (generate.py:56-125).  The graph comes from ``--edgelist`` (the reference's
``data/<name>/<name>.edgelist`` format, gcc/datasets/data_util.py:61-110), ``--ss-graph`` (a weighted co-author network
of the similarity-search task, ``data/panther/<name>.graph``: weight t = t parallel edges, embedded as the multigraph the
reference builds) or ``--graph-npz`` (row_ptr/col_idx); everything runs on the GPU (sampler, positional embedding, encoder).

Extra flags (not in the reference): --edgelist / --nodelabel / --ss-graph / --ss-dict / --graph-npz / --graphs-npz / --tudataset / --edge-multiplicity /
--batch-size / --wide-eval / --graph-batcher.  ``--wide-eval resident`` embeds with a wide GIN checkpoint (--hidden-size above 64, f32- or
bf16-trained) through one gcc_ginw_embed call per batch: bf16 layers resident in LDS, f32 readout (DESIGN.md section 7b has
the rounding rule the flag opts into); the default, ``chain``, is the any-width eval chain.  Graph-classification datasets (entire_graph=True, generate.py:75-82) come as ``--graphs-npz``: node_off
[G+1], row_ptr [N+1] (per-graph offsets restarting at 0 are rebuilt from node_off), col_idx (local ids)."""
import argparse

from gcc_amd.generate import DevicePipeline, run as main  # noqa: F401  (tests and callers use generate.main / generate.DevicePipeline)


if __name__ == "__main__":
    parser = argparse.ArgumentParser("argument for training")
    # fmt: off
    parser.add_argument("--load-path", type=str, help="path to load model")
    parser.add_argument("--dataset", type=str, default="dgl")
    parser.add_argument("--gpu", default=None, type=int, help="GPU id to use.")
    # ---- not in the reference: where the graph comes from
    parser.add_argument("--edgelist", type=str, default=None, help="<name>.edgelist of the reference's data folder")
    parser.add_argument("--nodelabel", type=str, default=None, help="<name>.nodelabel (only read to validate the node set)")
    parser.add_argument("--ss-graph", type=str, default=None, help="<name>.graph of the similarity-search networks (data/panther): 'x y t' lines, t parallel edges")
    parser.add_argument("--ss-dict", type=str, default=None, help="<name>.dict of --ss-graph (default: next to it)")
    parser.add_argument("--graph-npz", type=str, default=None, help="npz with row_ptr/col_idx of the simple symmetric graph")
    parser.add_argument("--graphs-npz", type=str, default=None, help="npz with node_off/row_ptr/col_idx of a list of small graphs (graph classification)")
    parser.add_argument("--tudataset", type=str, default=None, help="folder with the raw TU files <NAME>_A.txt, <NAME>_graph_indicator.txt, <NAME>_graph_labels.txt of --dataset (imdb-binary, imdb-multi, rdt-b, rdt-5k, collab)")
    parser.add_argument("--edge-multiplicity", type=int, default=0, help="copies of every edge in the reference's DGL graph (edge lists: detected; npz: default 2)")
    parser.add_argument("--batch-size", type=int, default=256)
    parser.add_argument("--graph-batcher", choices=["auto", "host", "device"], default="auto", help="--graphs-npz / --tudataset: assemble batches on the device (gcc_pack_graphs; auto on a GPU) or with the host loop")
    parser.add_argument("--tu-parse", choices=["host", "device"], default="host", help="--tudataset: parse the three TU files on the host (np.loadtxt) or on the device (gcc_text_ints_sep, gcc_tu_corpus); refused by gcc_amd.generate.run without --tudataset or with --graph-batcher host")
    parser.add_argument("--wide-eval", choices=["chain", "resident"], default="chain", help="wide GIN checkpoints: the any-width eval chain (f32 or the checkpoint's --encoder-dtype), or one LDS-resident bf16 call per batch (gcc_ginw_embed; f32 readout)")
    # fmt: on
    a = parser.parse_args()
    if a.graph_npz and not a.edge_multiplicity:
        a.edge_multiplicity = 2
    main(a)
