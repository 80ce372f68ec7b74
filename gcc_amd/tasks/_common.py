"""What the task modules share: the embedding-table reader, the reference's folds, the call of gcc_amd.generate.run that embeds a
corpus with a checkpoint, and the baseline tables (ProNE, GraphWave) on the device or by their NumPy restatements."""
from __future__ import annotations

import argparse
import os

import numpy as np

FOLDS = 10


def load_embedding(path):
    """a ``.npy`` table as ``generate.py`` writes it, or a ``.npz`` that holds one (its only array, or the one named "emb")"""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"embedding file not found: {path}")
    a = np.load(path)
    if isinstance(a, np.lib.npyio.NpzFile):
        keys = list(a.keys())
        if "emb" not in keys and len(keys) != 1:
            raise ValueError(f"{path}: expected one array or one named 'emb', found {keys}")
        a = a["emb" if "emb" in keys else keys[0]]
    if a.ndim != 2:
        raise ValueError(f"{path}: expected a [nodes, dim] table, found shape {a.shape}")
    return a


def fold_ids(labels, seed, folds=FOLDS):
    """fold_of_row [N] int32: the fold whose test side holds the row, from the reference's StratifiedKFold"""
    try:
        from sklearn.model_selection import StratifiedKFold
    except ImportError as e:                    # never another split silently: the folds are the reference's or none
        raise RuntimeError("graph classification needs scikit-learn (the reference's StratifiedKFold picks the folds)") from e
    fold = np.full(len(labels), -1, dtype=np.int32)
    for f, (_, test) in enumerate(StratifiedKFold(n_splits=folds, shuffle=True, random_state=seed).split(np.zeros(len(labels)), labels)):
        fold[test] = f
    return fold


def generate_namespace(load_path, dataset, device, batch_size, tu_parse="host", **source):
    """the arguments of gcc_amd.generate.run; ``source``: the members that name the input (edgelist and nodelabel, ss_graph and
    ss_dict, graphs_npz, tudataset), the others are None"""
    import torch

    dev = torch.device(device)
    inputs = dict(edgelist=None, nodelabel=None, ss_graph=None, ss_dict=None, graph_npz=None, graphs_npz=None, tudataset=None)
    if set(source) - set(inputs):
        raise TypeError(f"unknown input members {sorted(set(source) - set(inputs))}")
    inputs.update(source)
    return argparse.Namespace(load_path=load_path, dataset=dataset, gpu=dev.index if dev.type == "cuda" else None, edge_multiplicity=0,
                              batch_size=batch_size, wide_eval="chain", graph_batcher="auto", tu_parse=tu_parse, **inputs)


def checkpoint_table(load_path, dataset, device, batch_size, pipeline=None, tu_parse="host", **source):
    """the input embedded with the checkpoint ``load_path`` -> float32 [rows, hidden] on the host.  ``pipeline``: generate.py's
    seam for the emulator tests."""
    from ..generate import run

    return run(generate_namespace(load_path, dataset, device, batch_size, tu_parse=tu_parse, **source), pipeline=pipeline, save=False).numpy()


def baseline_table(kind, row_ptr, col_idx, d, device, engine=None, **kw):
    """the ``kind`` ("prone" / "graphwave") table of a CSR graph -> float32 [nodes, d] on the host: by the engine, or with ``device``
    "cpu" and no engine by the float64 NumPy restatement.  ``kw`` goes to ``embed`` / ``embed_numpy`` (ProNE's seed)."""
    if kind == "prone":
        from ..prone import ProNEEngine as Engine, embed_numpy
        key = "emb32"
    else:
        from ..graphwave import GraphWaveEngine as Engine, embed_numpy
        key = "chi32"
    if engine is None and str(device) == "cpu":
        return embed_numpy(row_ptr, col_idx, d, **kw)[key]
    engine = engine if engine is not None else Engine(device=device)
    res = engine.embed(row_ptr, col_idx, d, **kw)
    engine.check_status(res)
    return res[key].cpu().numpy()
