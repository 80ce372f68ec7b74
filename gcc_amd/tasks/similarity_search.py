"""Similarity search between two co-author networks (gcc/tasks/similarity_search.py:41-69 of the reference): the authors both
networks know are the keys; every key's row of the first embedding table is scored against the second table's rows of all
keys by cosine similarity, and Recall@k says how often the same author is among the k best.

    python -m gcc_amd.tasks.similarity_search --dataset kdd_icdm --emb-path-1 A.npy --emb-path-2 B.npy \\
        [--data-root data/panther] [--k 20 40] [--device cuda:0|cpu] [--save-topk out.npz]
    python -m gcc_amd.tasks.similarity_search --dataset kdd_icdm --load-path CKPT [--batch-size 256] [--save-emb DIR] ...
    python -m gcc_amd.tasks.similarity_search --dataset kdd_icdm --model graphwave [--hidden-size 64] [--save-emb DIR] ...

With ``--load-path`` the two tables need not exist: both networks are embedded on the device with the checkpoint (what
``generate.py --ss-graph`` does: the weighted network as the multigraph the reference builds, one row per node of the graph
file) and handed to the search without a trip through disk; ``--save-emb DIR`` stores them as ``DIR/<network>.npy``.

``--model graphwave`` is the reference's GraphWave baseline (gcc/models/emb/graphwave.py): both networks, as the multigraphs of
``read_ss_graph(csr=True)`` (one row per node of the graph file, parallel edges counted), are embedded by
gcc_amd.graphwave.GraphWaveEngine (gcc_amd/csrc/graphwave.hip) or, with ``--device cpu``, by its float64 NumPy restatement, and the
two tables are searched as above.  ``--model from_numpy`` (the default) is the search of given or checkpoint-made tables.

``--dataset a_b`` reads ``<data-root>/a.graph``, ``a.dict``, ``b.graph`` and ``b.dict`` (gcc_amd.ingest.read_ss_graph).  On a
GPU the search is one gcc_sim_search call (gcc_amd/simsearch.py); ``--device cpu`` runs the same rule in NumPy float64.  Among
equal scores the lower candidate column comes first (the reference's ``argsort()[::-1]`` leaves ties open), and a key counts
as found at k when fewer than k candidates come before its match.  Prints the reference's result line with the number of
queries added.  ``--save-topk`` stores names, columns and scores of each query's max(k) best candidates."""
from __future__ import annotations

import argparse
import os

import numpy as np

from ..ingest import read_ss_graph
from ._common import baseline_table, checkpoint_table, load_embedding  # noqa: F401  (load_embedding: importable from here)


def select_keys(dict_1, dict_2, rows_1, rows_2):
    """The names both dicts hold whose rows exist in both tables (in sorted order: the reference's set order is arbitrary)
    -> (names, q_rows int32, c_rows int32, target int32).  Candidate column j is ``c_rows[j]``; a query's target is the column
    of its own row of table 2 -- with a row listed twice (two names, one id), the last column that lists it."""
    names = sorted(x for x in set(dict_1) & set(dict_2) if dict_1[x] < rows_1 and dict_2[x] < rows_2)
    q_rows = np.array([dict_1[x] for x in names], dtype=np.int32)
    c_rows = np.array([dict_2[x] for x in names], dtype=np.int32)
    last = {int(r): j for j, r in enumerate(c_rows)}
    target = np.array([last[int(r)] for r in c_rows], dtype=np.int32)
    return names, q_rows, c_rows, target


def search_numpy(emb_1, emb_2, q_rows, c_rows, target, k, chunk=1024):
    """float64 on the host, the order rule of gcc_sim_search: -> (greater, equal_before, topk_col, topk_score)"""
    q, c = emb_1[q_rows].astype(np.float64), emb_2[c_rows].astype(np.float64)
    for name, rows in (("--emb-path-1", q), ("--emb-path-2", c)):
        if rows.size and (np.linalg.norm(rows, axis=1) == 0).any():
            raise RuntimeError(f"{name}: a selected row has norm 0 (the reference would divide by zero)")
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    mq, mc = len(q), len(c)
    kk = min(k, mc)
    greater, equal_before = np.zeros(mq, np.int64), np.zeros(mq, np.int64)
    topk_col, topk_score = np.full((mq, k), -1, np.int32), np.full((mq, k), -np.inf, np.float32)
    cols = np.arange(mc)
    for q0 in range(0, mq, chunk):
        s = q[q0: q0 + chunk] @ c.T
        t = target[q0: q0 + chunk]
        st = s[np.arange(len(s)), t][:, None]
        greater[q0: q0 + chunk] = (s > st).sum(1)
        equal_before[q0: q0 + chunk] = ((s == st) & (cols[None, :] < t[:, None])).sum(1)
        if kk:
            order = np.argsort(-s, axis=1, kind="stable")[:, :kk]          # stable: equal scores keep their column order
            topk_col[q0: q0 + chunk, :kk] = order
            topk_score[q0: q0 + chunk, :kk] = np.take_along_axis(s, order, 1)
    return greater, equal_before, topk_col, topk_score


def evaluate(emb_1, emb_2, dict_1, dict_2, ks=(20, 40), device="cpu", with_topk=False, engine=None):
    """-> (result {"Recall @ k": ..., "queries": n}, detail dict(names, target, greater, equal_before[, topk_col, topk_score])).
    ``engine``: a gcc_amd.simsearch.SimilarityEngine (injectable for the emulator tests); the NumPy path when ``device`` is
    "cpu" and no engine is given."""
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1:
        raise ValueError("--k needs positive values")
    names, q_rows, c_rows, target = select_keys(dict_1, dict_2, emb_1.shape[0], emb_2.shape[0])
    if not names:
        raise ValueError("the two dicts share no name whose rows exist in both embedding tables")
    k = max(ks) if with_topk else 0
    if engine is None and str(device) == "cpu":
        greater, equal_before, topk_col, topk_score = search_numpy(emb_1, emb_2, q_rows, c_rows, target, k)
    else:
        import torch

        from .. import _cabi
        from ..simsearch import SimilarityEngine

        if k > _cabi.SIM_MAX_K:
            raise ValueError(f"--save-topk on the device holds up to {_cabi.SIM_MAX_K} candidates per query (max --k is {k})")
        engine = engine if engine is not None else SimilarityEngine()
        dev = torch.device(device)
        put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)        # noqa: E731
        res = engine.search(put(emb_1, torch.float32), put(emb_2, torch.float32), put(q_rows, torch.int32),
                            put(c_rows, torch.int32), put(target, torch.int32), k=k, normalize=True)
        engine.check_status(res)
        greater, equal_before = res["greater"].cpu().numpy().astype(np.int64), res["equal_before"].cpu().numpy().astype(np.int64)
        topk_col, topk_score = res["topk_col"].cpu().numpy(), res["topk_score"].cpu().numpy()
    before = greater + equal_before
    result = {f"Recall @ {kk}": int((before < kk).sum()) / len(names) for kk in ks}
    result["queries"] = len(names)
    detail = dict(names=names, target=target, greater=greater, equal_before=equal_before)
    if with_topk:
        detail.update(topk_col=topk_col, topk_score=topk_score)
    return result, detail


def load_dicts(data_root, dataset):
    parts = dataset.split("_")
    if len(parts) != 2 or not all(parts):
        raise ValueError(f"unknown dataset {dataset!r}: expected <network 1>_<network 2>, e.g. kdd_icdm")
    dicts = []
    for name in parts:
        graph_path, dict_path = os.path.join(data_root, name + ".graph"), os.path.join(data_root, name + ".dict")
        for p in (graph_path, dict_path):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"unknown dataset {dataset!r}: {p} not found")
        dicts.append(read_ss_graph(graph_path, dict_path)["name_dict"])
    return dicts


def embed_networks(data_root, dataset, load_path, batch_size=256, device="cuda:0", pipeline=None):
    """Both networks of ``dataset`` embedded with the checkpoint ``load_path`` (gcc_amd.generate.run on ``--ss-graph``) ->
    [table 1, table 2], float32 [nodes of the graph file, hidden].  ``pipeline``: generate.py's seam for the emulator tests."""
    return [checkpoint_table(load_path, name, device, batch_size, pipeline, ss_graph=os.path.join(data_root, name + ".graph"),
                             ss_dict=os.path.join(data_root, name + ".dict")) for name in dataset.split("_")]


def embed_graphwave(data_root, dataset, hidden_size=64, device="cuda:0", graphwave_engine=None):
    """Both networks of ``dataset`` as GraphWave tables -> [table 1, table 2], float32 [nodes of the graph file, hidden_size]"""
    from ..graphwave import check_width

    check_width(hidden_size)
    tables = []
    for name in dataset.split("_"):
        g = read_ss_graph(os.path.join(data_root, name + ".graph"), os.path.join(data_root, name + ".dict"), csr=True)
        tables.append(baseline_table("graphwave", g["row_ptr"], g["col_idx"], hidden_size, device, graphwave_engine))
    return tables


def main(argv=None, pipeline=None, engine=None, graphwave_engine=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset", required=True, help="<network 1>_<network 2>, e.g. kdd_icdm")
    ap.add_argument("--emb-path-1", default=None)
    ap.add_argument("--emb-path-2", default=None)
    ap.add_argument("--load-path", default=None, help="checkpoint: embed both networks on the device instead of reading --emb-path-1/-2")
    ap.add_argument("--batch-size", type=int, default=256, help="--load-path: nodes embedded per batch")
    ap.add_argument("--save-emb", default=None, metavar="DIR", help="--load-path / --model graphwave: store the two tables as DIR/<network>.npy")
    ap.add_argument("--model", default="from_numpy", choices=["from_numpy", "graphwave"],
                    help="the reference's option: from_numpy (tables that exist or --load-path makes) or graphwave (the baseline)")
    ap.add_argument("--hidden-size", type=int, default=None, help="--model graphwave: the tables' width (default 64, a multiple of 4); else checked against the tables' width")
    ap.add_argument("--data-root", default=os.path.join("data", "panther"))
    ap.add_argument("--k", type=int, nargs="+", default=[20, 40])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--save-topk", default=None, metavar="OUT.npz")
    a = ap.parse_args(argv)
    if a.model == "graphwave":
        if a.load_path is not None or a.emb_path_1 is not None or a.emb_path_2 is not None:
            ap.error("--model graphwave computes the tables: it takes neither --emb-path-1/-2 nor --load-path")
        hidden = 64 if a.hidden_size is None else a.hidden_size
        if hidden % 4 != 0 or not 4 <= hidden <= 256:
            ap.error(f"--model graphwave: --hidden-size {hidden} must be a multiple of 4 in 4..256")
    elif a.load_path is None and (a.emb_path_1 is None or a.emb_path_2 is None):
        ap.error("pass --emb-path-1 and --emb-path-2, or --load-path to embed the two networks")
    dict_1, dict_2 = load_dicts(a.data_root, a.dataset)
    if a.model == "graphwave" or a.load_path is not None:
        if a.model == "graphwave":
            emb_1, emb_2 = embed_graphwave(a.data_root, a.dataset, hidden, a.device, graphwave_engine)
        else:
            emb_1, emb_2 = embed_networks(a.data_root, a.dataset, a.load_path, a.batch_size, a.device, pipeline)
        if a.save_emb is not None:
            os.makedirs(a.save_emb, exist_ok=True)
            for name, emb in zip(a.dataset.split("_"), (emb_1, emb_2)):
                np.save(os.path.join(a.save_emb, name + ".npy"), emb)
    else:
        emb_1, emb_2 = load_embedding(a.emb_path_1), load_embedding(a.emb_path_2)
    if a.hidden_size is not None and not emb_1.shape[1] == emb_2.shape[1] == a.hidden_size:
        ap.error(f"--hidden-size {a.hidden_size}, but the tables have {emb_1.shape[1]} and {emb_2.shape[1]} columns")
    result, detail = evaluate(emb_1, emb_2, dict_1, dict_2, a.k, a.device, with_topk=a.save_topk is not None, engine=engine)
    if a.save_topk is not None:
        names = np.array(detail["names"])
        cols = detail["topk_col"]
        np.savez(a.save_topk, names=names, target=detail["target"], topk_col=cols, topk_score=detail["topk_score"],
                 topk_name=np.where(cols >= 0, names[np.maximum(cols, 0)], ""))
    print(result)
    return result


if __name__ == "__main__":
    main()
