"""``python -m gcc_amd.x2dgl --graph-dir D --save-file F.bin``: raw edge files -> the pre-training corpus ``train.py --dgl-file``
reads.  The reference's converter (gcc/utils/x2dgl.py) needs DGL; this one builds every graph on the device
(gcc_amd.graph_build, gcc_graph_build) by the same rule and writes the same container (gcc_amd.ingest.write_dgl_graphs).

    --graph-dir D      the folder of ``.lscc`` files (gcc_amd.ingest.read_lscc)
    --save-file F      the DGL ``.bin`` file to write, with the label ``graph_sizes``
    --files a,b,...    file names inside D; default: the reference's six networks (those that exist in D)
    --embed-dim N      accepted and ignored: the reference requires it and never reads it
    --device           cuda:0 (default) or cpu (the NumPy restatement of the rule: ``build_csr_numpy``)
    --parse            host (default: gcc_amd.ingest.read_lscc) or device (gcc_amd.text_ingest: the file's bytes are parsed on the
                       device and the pairs never visit the host); not with --device cpu
    --save-npz DIR     additionally one ``<file name>.npz`` (row_ptr, col_idx) per graph, for ``--graph-npz``

Graphs are written by node count descending; ties go by file name ascending (the reference leaves ties to the directory's order)."""
from __future__ import annotations

import argparse
import logging
import os

import numpy as np

from . import ingest
from .corpus import REFERENCE_FILES, build_corpus, build_graph  # noqa: F401  (the names this module has always had)

logger = logging.getLogger(__name__)


def main(argv=None, engine=None, text_engine=None):
    """``engine`` / ``text_engine``: a GraphBuildEngine to build with and a TextIngestEngine to parse with (the emulator tests inject
    theirs) -> the graphs in the order written"""
    parser = argparse.ArgumentParser("argument for x2dgl")
    parser.add_argument("--graph-dir", type=str, required=True, help="dir to load graphs")
    parser.add_argument("--save-file", type=str, required=True, help="file to save graphs")
    parser.add_argument("--embed-dim", type=int, default=None, help="accepted and ignored (the reference never reads it)")
    parser.add_argument("--files", type=str, default=None, help="comma-separated file names inside --graph-dir (default: the reference's six)")
    parser.add_argument("--device", type=str, default="cuda:0", help="cuda:0, or cpu for the NumPy path")
    parser.add_argument("--parse", type=str, default="host", choices=("host", "device"), help="where the edge files are parsed")
    parser.add_argument("--save-npz", type=str, default=None, help="folder for one row_ptr / col_idx npz per graph")
    args = parser.parse_args(argv)
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s - %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO)
    if args.parse == "device" and engine is None and text_engine is None and args.device == "cpu":
        parser.error("--parse device parses on the device: not with --device cpu, which reads with the host parser")
    graphs = build_corpus(args.graph_dir, args.files.split(",") if args.files is not None else None, args.device, engine, parse=args.parse,
                          text_engine=text_engine)
    sizes = np.array([g["counts"][0] for g in graphs], dtype=np.int64)
    for i, g in enumerate(graphs):
        print(i, f"{g['name']}: {g['counts'][0]} nodes, {g['counts'][1]} edges", int(sizes[i]))
    logger.info("save graphs to %s", args.save_file)
    ingest.write_dgl_graphs(args.save_file, [(g["row_ptr"], g["col_idx"]) for g in graphs], labels={"graph_sizes": sizes})
    if args.save_npz:
        os.makedirs(args.save_npz, exist_ok=True)
        for g in graphs:
            np.savez(os.path.join(args.save_npz, g["name"] + ".npz"), row_ptr=g["row_ptr"], col_idx=g["col_idx"])
    return graphs


if __name__ == "__main__":
    main()
