"""TU dataset text on the device: ``<NAME>_A.txt``, ``_graph_indicator.txt`` and ``_graph_labels.txt`` -> the resident corpus of
``DeviceGraphCorpus`` (gcc_text_ints_sep, gcc_amd/csrc/text_ingest.hip; gcc_tu_corpus, gcc_amd/csrc/tu_corpus.hip).

The host reader (``gcc_amd.ingest.read_tudataset``) makes three ``np.loadtxt`` calls, seven validation passes, a ``lexsort`` and one
slice per graph, and ``DeviceGraphCorpus.__init__`` concatenates the slices again.  Here the three files go to the device as bytes
(``TextIngestEngine.upload``) and stay there:

    1. three count-only calls (``max_tokens = 0``, no output) give the files' token counts: one host read sizes every buffer;
    2. ``A.txt`` is tokenised with ``extra_sep=44, fields=2, keep=2, line_records=1``, the other two with ``fields=1, line_records=1``;
    3. ``gcc_tu_corpus`` builds node_first, edge_first, row_ptr, col_idx, seed_local and the re-indexed labels;
    4. one packed host read brings the counts, the four status words with their offsets, node_first, edge_first and the labels.

Errors are the host reader's ``ValueError``s word for word, raised in its order (the lowest bit of gcc_tu_corpus' status word).  A
token of ``A.txt`` outside int32 is stored as 0 and so raises the host's "node id out of range in A.txt" where the host would.  Three
errors exist only here, each with the file and the byte offset: a token that is no integer, a line of the wrong shape, and an
indicator or label value outside int32.

Differences from ``np.loadtxt``:

    * ``#`` comment lines are not skipped: they are errors here;
    * ``1,,2`` and ``1 2`` are read as two fields (the comma is one more separator; empty fields do not exist);
    * a token with an underscore (``1_0``) is not an integer;
    * an empty ``A.txt`` is an edge-free dataset (``np.loadtxt`` gives it the shape (0, 1) and the host reader stops with an
      IndexError at its second column);
    * an empty ``graph_indicator.txt`` or ``graph_labels.txt`` is an error by name (the host returns an empty dataset or fails later).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _cabi
from ._engine import CabiEngine
from .ingest import TU_NAMES
from .text_ingest import TextIngestEngine

COMMA = 44
TU_ERRORS = (
    (_cabi.STATUS_TU_DESCENDS, "graph_indicator must be non-decreasing (nodes of a graph are contiguous in the TU format)"),
    (_cabi.STATUS_TU_GRAPH_COUNT, None),              # (carries two numbers)
    (_cabi.STATUS_TU_BAD_ID, "node id out of range in A.txt"),
    (_cabi.STATUS_TU_SELF_LOOP, "self loops are not supported by the sampler contract (x2dgl.py:41-42 removes them)"),
    (_cabi.STATUS_TU_CROSS_GRAPH, "an edge connects two different graphs"),
    (_cabi.STATUS_TU_REPEATED, "repeated adjacency entries: a general multigraph is not supported"),
    (_cabi.STATUS_TU_ASYMMETRIC, "the adjacency is not symmetric"),
)
_HEAD = 48                                            # int32 words in front of node_first in the packed report


def tu_error(status, graphs, num_labels):
    """the host reader's message for the lowest set bit of gcc_tu_corpus' status word, or None"""
    for bit, text in TU_ERRORS:
        if status & bit:
            return text if text is not None else f"{graphs} graphs in graph_indicator but {num_labels} graph labels"
    return None


class TUIngestEngine(CabiEngine):
    """C-ABI calls of the TU reader.  ``lib``/``ptr`` are injectable for the emulator tests only."""

    def __init__(self, lib=None, ptr=None, device="cuda:0", text_engine=None):
        super().__init__(lib, ptr, device)
        self.text = text_engine if text_engine is not None else TextIngestEngine(self.lib, self.ptr, device)

    # ------------------------------------------------------------------ the bare call
    def corpus_into(self, pairs, indicator, graph_labels, num_lines, out, workspace_bytes=None):
        """gcc_tu_corpus with the outputs as the caller allocated them (``out``: node_first, edge_first, row_ptr, col_idx,
        seed_local, labels, counts int64 [8], status zeroed int32 [1]; a None stays NULL).  Enqueued on torch's current stream."""
        p = lambda t: self.ptr(t) if t is not None and t.numel() else None           # noqa: E731
        a = _cabi.GccTuCorpusArgs()
        a.pairs, a.indicator, a.graph_labels = p(pairs), p(indicator), p(graph_labels)
        a.num_nodes = int(indicator.numel()) if indicator is not None else 0
        a.num_lines = int(num_lines)
        a.num_labels = int(graph_labels.numel()) if graph_labels is not None else 0
        for name in ("node_first", "edge_first", "row_ptr", "col_idx", "seed_local", "labels", "counts"):
            setattr(a, name, p(out.get(name)))
        status = out["status"]
        need = _cabi.size_query(self.lib, "gcc_tu_corpus_workspace_bytes", a.num_nodes, a.num_lines, a.num_labels)
        self.invoke("gcc_tu_corpus", a, self.workspace(need, status.device), status, workspace_bytes)

    def _buffers(self, N, m, L, device):
        """the outputs of one build; counts, the status word, node_first, edge_first and labels are views of ``report`` (int32), so
        that one host read brings them all"""
        i32 = dict(dtype=torch.int32, device=device)
        report = torch.zeros(_HEAD + 3 * L + 2, **i32)
        out = dict(report=report, counts=report[:16].view(torch.int64), tokens=report[16:46].view(torch.int64).view(3, 5),
                   status=report[46:47], node_first=report[_HEAD:_HEAD + L + 1],
                   edge_first=report[_HEAD + L + 1:_HEAD + 2 * L + 2], labels=report[_HEAD + 2 * L + 2:],
                   row_ptr=torch.empty(N + 1, **i32), col_idx=torch.zeros(1, **i32) if m == 0 else torch.empty(m, **i32),
                   seed_local=torch.empty(L, **i32))
        return out

    def corpus(self, pairs, indicator, graph_labels):
        """``pairs`` int32 [m, 2] (the 1-based ids of A.txt, any line order), ``indicator`` int32 [N], ``graph_labels`` int32 [L], all
        on the device -> dict(node_first, edge_first, row_ptr, col_idx, seed_local, labels, counts int64 [8], status int32 [1],
        report), all on the device; nothing is read back."""
        for name, t, dims in (("pairs", pairs, 2), ("indicator", indicator, 1), ("graph_labels", graph_labels, 1)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != dims or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous int32 tensor of {dims} dimension(s)")
            self.require_device(t)
        if pairs.shape[1] != 2:
            raise ValueError("pairs must be [m, 2]")
        N, m, L = int(indicator.numel()), int(pairs.shape[0]), int(graph_labels.numel())
        out = self._buffers(max(N, 0), m, max(L, 0), indicator.device)
        self.corpus_into(pairs, indicator, graph_labels, m, out)
        return out

    # ------------------------------------------------------------------ the three files
    def read_tudataset(self, folder, name, chunk_bytes=64 << 20):
        """``gcc_amd.ingest.read_tudataset`` with the text on the device -> dict(graph_labels int64 [G] on the host, num_labels,
        corpus=dict(node_first, row_ptr, col_idx, seed_local, labels on the device; sizes, entries int64 on the host), counts).
        ``corpus`` is what ``DeviceGraphCorpus.from_device`` takes.  Raises the host reader's ValueErrors (see the module docstring
        for the differences)."""
        base = os.path.join(folder, TU_NAMES.get(name, name) + "_")
        paths = [base + "A.txt", base + "graph_indicator.txt", base + "graph_labels.txt"]
        extra = (COMMA, 0, 0)
        fields = (2, 1, 1)
        texts = [self.text.upload(p, chunk_bytes) for p in paths]
        device = texts[0][0].device
        # 1. the token counts: one host read
        counted = torch.zeros(3, 5, dtype=torch.int64, device=device)
        for k, (text, nbytes) in enumerate(texts):
            if nbytes:
                self.text.ints_sep_into(text, nbytes, 0, 0, fields[k], fields[k], None, counted[k, :4], counted[k, 4:].view(torch.int32)[:1],
                                        extra_sep=extra[k])
        tokens = [int(x) for x in counted[:, 0].cpu()]
        for k in (1, 2):
            if tokens[k] == 0:
                raise ValueError(f"{paths[k]}: the file holds no integer")
        for k in range(3):
            if tokens[k] >= 2 ** 31 - 1:
                raise ValueError(f"{paths[k]}: {tokens[k]} tokens do not fit int32 offsets")
        m, N, L = (tokens[0] + 1) // 2, tokens[1], tokens[2]        # (an odd count: the last line is short, found below)
        out = self._buffers(N, m, L, device)
        # 2. the integers
        pairs = torch.zeros(m, 2, dtype=torch.int32, device=device)
        indicator = torch.empty(N, dtype=torch.int32, device=device)
        raw = torch.empty(L, dtype=torch.int32, device=device)
        for k, (dst, count) in enumerate(((pairs, 2 * m), (indicator, N), (raw, L))):
            text, nbytes = texts[k]
            if count:
                self.text.ints_sep_into(text, nbytes, 0, count, fields[k], fields[k], dst, out["tokens"][k, :4],
                                        out["tokens"][k, 4:].view(torch.int32)[:1], extra_sep=extra[k], line_records=1)
        # 3. the build (on zeros where a token was refused: every id is checked before it is used)
        self.corpus_into(pairs, indicator, raw, m, out)
        # 4. one packed read
        rep = out["report"].cpu()
        counts = rep[:16].view(torch.int64).numpy().copy()
        tok = rep[16:46].view(torch.int64).view(3, 5)
        for k in range(3):
            self._raise_text_error(paths[k], texts[k], [int(x) for x in tok[k, :4]], int(tok[k, 4:].view(torch.int32)[0]), k == 0)
        message = tu_error(int(rep[46]), int(counts[0]), L)
        if message is not None:
            raise ValueError(message)
        node_first = rep[_HEAD:_HEAD + L + 1].numpy().astype(np.int64)
        edge_first = rep[_HEAD + L + 1:_HEAD + 2 * L + 2].numpy().astype(np.int64)
        labels = rep[_HEAD + 2 * L + 2:].numpy().astype(np.int64)
        corpus = dict(node_first=out["node_first"], row_ptr=out["row_ptr"], col_idx=out["col_idx"], seed_local=out["seed_local"],
                      labels=out["labels"], sizes=np.diff(node_first), entries=np.diff(edge_first), report=out["report"])
        return dict(graph_labels=labels, num_labels=int(counts[1]), corpus=corpus, counts=counts)

    @staticmethod
    def _raise_text_error(path, text_nbytes, summary, status, is_pairs):
        """the three errors of this route alone, in the order not-an-integer, line shape, range"""
        text, nbytes = text_nbytes
        _, bad_at, range_at, shape_at = summary

        def token_at(at):
            return text[at:min(at + 64, nbytes)].cpu().numpy().tobytes().replace(b",", b" ").split()[0][:40]

        if status & _cabi.STATUS_TEXT_NOT_INTEGER:
            raise ValueError(f"{path}: a line holds something other than integers (the token {token_at(bad_at)!r} at byte {bad_at})")
        want = "two integers `u, v`" if is_pairs else "one integer"
        if status & _cabi.STATUS_TEXT_LINE_SHAPE:
            raise ValueError(f"{path}: every line must hold {want} (the token {token_at(shape_at)!r} at byte {shape_at})")
        if status & _cabi.STATUS_TEXT_SHORT:         # an odd number of tokens whose last line holds one
            tail_at = max(nbytes - 4096, 0)
            tail = text[tail_at:nbytes].cpu().numpy().tobytes().rstrip(b"\t\n\x0b\x0c\r ,")
            at = tail_at + len(tail) - len(tail.replace(b",", b" ").split()[-1])
            raise ValueError(f"{path}: every line must hold {want} (the token {token_at(at)!r} at byte {at})")
        if status & _cabi.STATUS_TEXT_INT32_RANGE and not is_pairs:
            raise ValueError(f"{path}: a value does not fit int32 (the token {token_at(range_at)!r} at byte {range_at})")
