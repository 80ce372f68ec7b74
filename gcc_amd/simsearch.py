"""Similarity search on the device: cosine scores of every query row against every candidate row, the rank counts behind
Recall@k and the k best candidates of each query (gcc_sim_search, gcc_amd/csrc/simsearch.hip) -- what the reference's
gcc/tasks/similarity_search.py:41-69 computes with one argsort per query, without a [queries, candidates] score matrix.

A query's candidates are ordered by score descending, then column ascending (the reference's ``argsort()[::-1]`` leaves ties
open; this is the documented choice).  Recall@k comes from the counts ``greater + equal_before < k`` and never from the lists,
so the two can be checked against each other.
"""
from __future__ import annotations

import torch

from . import _cabi
from ._engine import CabiEngine

STATUS_BITS = {_cabi.STATUS_SIM_ZERO_ROW: "a selected row has norm 0 (the reference would divide by zero)",
               _cabi.STATUS_SIM_BAD_INDEX: "a q_idx / c_idx entry outside its table or a target outside [-1, mc)"}


class SimilarityEngine(CabiEngine):
    """C-ABI calls of the similarity search.  ``lib``/``ptr`` are injectable for the emulator tests only."""

    def search(self, emb_q, emb_c, q_idx=None, c_idx=None, target=None, k=0, normalize=True, splits=0, stream=None):
        """emb_q [rows_q, D] / emb_c [rows_c, D]: float32, unit stride along D (a row stride larger than D is served).
        q_idx / c_idx: int32 rows of the tables (None: every row in order); target: int32 [mq], the candidate column of each
        query's true match or -1.  -> dict(greater, equal_before int32 [mq]; target_score float32 [mq]; topk_col int32 /
        topk_score float32 [mq, k]; status int32 [1]; mq, mc, k).  Nothing is read back here: see check_status / recall_at_k."""
        a = _cabi.GccSimArgs()
        a.emb_q, a.rows_q, D, a.ld_q = self.table(emb_q, "emb_q")
        a.emb_c, a.rows_c, Dc, a.ld_c = self.table(emb_c, "emb_c")
        if D != Dc:
            raise ValueError(f"emb_q has {D} columns, emb_c {Dc}")
        dev = emb_q.device
        for name, t in (("q_idx", q_idx), ("c_idx", c_idx), ("target", target)):
            if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous int32 vector")
        mq = int(q_idx.numel()) if q_idx is not None else int(emb_q.shape[0])
        mc = int(c_idx.numel()) if c_idx is not None else int(emb_c.shape[0])
        if target is not None and target.numel() != mq:
            raise ValueError(f"target has {target.numel()} entries for {mq} queries")
        k = int(k)
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        served = mq > 0 and mc > 0             # a call that launches writes every entry; otherwise the padding is the answer
        def fresh(shape, fill, **kw):
            return torch.empty(shape, **kw) if served else torch.full(shape, fill, **kw)

        out = dict(greater=fresh((mq,), -1, **i32), equal_before=fresh((mq,), -1, **i32),
                   target_score=fresh((mq,), float("nan"), **f32),
                   topk_col=fresh((mq, max(k, 0)), -1, **i32), topk_score=fresh((mq, max(k, 0)), float("-inf"), **f32),
                   status=torch.zeros(1, **i32), mq=mq, mc=mc, k=k)
        nbytes = _cabi.size_query(self.lib, "gcc_sim_workspace_bytes", mq, mc, D, k, int(splits))
        if not served:                         # nothing to search: the outputs keep their padding
            return out
        a.q_idx, a.c_idx, a.target = self.ptr(q_idx), self.ptr(c_idx), self.ptr(target)
        a.mq, a.mc, a.D, a.k, a.normalize, a.splits = mq, mc, D, k, int(bool(normalize)), int(splits)
        a.greater, a.equal_before, a.target_score = self.ptr(out["greater"]), self.ptr(out["equal_before"]), self.ptr(out["target_score"])
        if k > 0:
            a.topk_col, a.topk_score = self.ptr(out["topk_col"]), self.ptr(out["topk_score"])
        self.invoke("gcc_sim_search", a, self.workspace(nbytes, dev), out["status"], stream=stream)
        return out

    @staticmethod
    def recall_at_k(result, ks):
        """{k: hits / queries with a target}; a query is a hit at k when fewer than k candidates come before its match.
        One host read of the two counters."""
        counts = torch.stack([result["greater"], result["equal_before"]]).cpu()
        have = counts[0] >= 0
        n = int(have.sum())
        before = (counts[0] + counts[1])[have]
        return {int(k): (int((before < int(k)).sum()) / n if n else float("nan")) for k in ks}

    @staticmethod
    def check_status(result, allow_zero_rows=False):
        """Raises and names the bits of the call's status word (one host read).  A zero row raises unless allowed: the
        reference would divide by zero there; here it scores 0 against everything."""
        CabiEngine.raise_status(result, "gcc_sim_search", STATUS_BITS, _cabi.STATUS_SIM_ZERO_ROW if allow_zero_rows else 0)
