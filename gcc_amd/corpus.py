"""A folder of raw edge files -> the pre-training corpus, every graph built on the device (gcc_amd.graph_build, gcc_graph_build) by
the reference converter's rule.  ``python -m gcc_amd.x2dgl`` downloads the result and writes the DGL ``.bin``;
``train.py --graph-dir`` keeps it where it was built (``keep_on_device=True``) and hands it to the sampler.

Graphs come out by node count descending; ties go by file name ascending (the reference leaves ties to the directory's order)."""
from __future__ import annotations

import logging
import os

import numpy as np

from . import ingest
from .graph_build import BUILD_STATUS_BITS, build_csr_numpy

logger = logging.getLogger("gcc_amd.x2dgl")             # (the converter's log lines keep the name they have always carried)

# x2dgl.py:88-97
REFERENCE_FILES = ("ca-DBLP-NetRep.txt.lpm.lscc", "ca-DBLP-SNAP.txtu.lpm.lscc", "ca-IMDB-NetRep.txt.lpm.lscc",
                   "soc-Academia-NetRep.txt.lpm.lscc", "soc-LiveJournal1-d-SNAP.txtu.lpm.lscc", "soc-Facebook1-NetRep.txt.lpm.lscc")


def build_graph(path, device="cuda:0", engine=None, keep_on_device=False, parse="host", text_engine=None):
    """one file -> dict(name, row_ptr, col_idx, counts): read, built, and the reference's line logged.  row_ptr / col_idx are numpy
    int32, or with ``keep_on_device`` the int32 device tensors of the build.  ``parse``: "host" (``ingest.read_lscc``) or "device"
    (``gcc_amd.text_ingest``: the file's bytes go to the device and the pairs never visit the host); ``text_engine``: a
    TextIngestEngine to parse with (the emulator tests inject theirs)"""
    if parse not in ("host", "device"):
        raise ValueError(f"parse {parse!r}: 'host' or 'device'")
    if parse == "device":
        if engine is None and text_engine is None and str(device) == "cpu":
            raise ValueError("parse='device' needs a device: --device cpu is the NumPy restatement and reads with the host parser")
        if text_engine is None:
            from .text_ingest import TextIngestEngine

            text_engine = TextIngestEngine(device=device)
        if engine is None:
            from .graph_build import GraphBuildEngine

            engine = GraphBuildEngine(device=device)
        n, pairs = text_engine.read_lscc(path)
    else:
        n, pairs = ingest.read_lscc(path)
    logger.info("processing %s", path)
    logger.info("raw file has %d nodes and %d edges", n, len(pairs))
    if engine is None and str(device) == "cpu":
        if keep_on_device:
            raise ValueError("keep_on_device needs a device: --device cpu is the NumPy restatement")
        out = build_csr_numpy(pairs, n)
    else:
        if engine is None:
            from .graph_build import GraphBuildEngine

            engine = GraphBuildEngine(device=device)
        out = engine.build(pairs, n)
        keep = ("row_ptr", "col_idx") if keep_on_device else ()
        out = {k: (v.cpu().numpy() if hasattr(v, "cpu") and k not in keep else v) for k, v in out.items()}
    if int(out["status"][0]):
        raise SystemExit(f"{path}: " + "; ".join(text for bit, text in BUILD_STATUS_BITS.items() if int(out["status"][0]) & bit))
    counts = [int(c) for c in out["counts"]]
    # (the reference counts the two slots of a self-loop line: x2dgl.py:67)
    logger.info("%d nodes, %d edges, %d self-loop(s) removed, %d zero-degree node(s) removed", counts[0], counts[1], 2 * counts[2], counts[4])
    if keep_on_device:
        return dict(name=os.path.basename(path), row_ptr=out["row_ptr"], col_idx=out["col_idx"], counts=counts)
    return dict(name=os.path.basename(path), row_ptr=np.asarray(out["row_ptr"]), col_idx=np.asarray(out["col_idx"]), counts=counts)


def build_corpus(graph_dir, files=None, device="cuda:0", engine=None, keep_on_device=False, parse="host", text_engine=None):
    """``files``: names inside ``graph_dir`` (default: the reference's six networks, those that exist there) -> the graphs
    (``build_graph``'s dicts) in corpus order.  A missing file, an empty selection and a graph without an edge end the program by
    name, as the converter always has.  ``parse`` / ``text_engine``: as in ``build_graph``."""
    if parse not in ("host", "device"):
        raise ValueError(f"parse {parse!r}: 'host' or 'device'")
    if parse == "device" and engine is None and text_engine is None and str(device) == "cpu":
        raise ValueError("parse='device' needs a device: --device cpu is the NumPy restatement and reads with the host parser")
    if files is not None:
        names = [x for x in files if x]
        missing = [x for x in names if not os.path.isfile(os.path.join(graph_dir, x))]
        if missing:
            raise SystemExit(f"--files: not in {graph_dir}: {', '.join(missing)}")
    else:
        names = [x for x in REFERENCE_FILES if os.path.isfile(os.path.join(graph_dir, x))]
    if not names:
        raise SystemExit(f"no graph file to convert in {graph_dir} (the reference's names: {', '.join(REFERENCE_FILES)}; others with --files)")
    graphs = [build_graph(os.path.join(graph_dir, x), device, engine, keep_on_device, parse, text_engine) for x in names]
    empty = [g["name"] for g in graphs if g["counts"][0] == 0]
    if empty:
        raise SystemExit(f"no edge is left in {', '.join(empty)}: a graph without nodes cannot be sampled")
    graphs.sort(key=lambda g: (-g["counts"][0], g["name"]))
    return graphs
