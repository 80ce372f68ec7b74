"""Edge-list text on the device: the bytes of a ``.lscc`` file -> (n, pairs int32 [m, 2] in HBM), what
``GraphBuildEngine.build`` takes (gcc_text_line_ends / gcc_text_ints, gcc_amd/csrc/text_ingest.hip).

The host reader (``gcc_amd.ingest.read_lscc``) makes one Python ``bytes`` object per token; here the file goes to the device in
chunks through two pinned staging buffers, and two calls turn it into the pair table:

    1. ``n`` is read on the host from the first line (it lies in the first chunk: its newline is looked for in the first 4,096 bytes);
    2. ``line_ends`` for the lines ``n`` and ``n + 1``: one host read brings two offsets and the newline total;
    3. the ``<word> m`` line between them is copied back and parsed by the host reader's own rule;
    4. ``ints`` from the byte after that line: ``max_tokens = 3 m``, ``fields = 3``, ``keep = 2`` (``w`` of ``u v w`` is checked for
       syntax and dropped);
    5. one host read of the summary and the status word.

The token rule is ``bytes.split()``'s (separators 9, 10, 11, 12, 13, 32); line structure is not looked at in the body.  Errors are
``ValueError``s in the host reader's words.

Two differences from the host reader:

    * the device reader ignores everything after the ``3 m``-th token; the host converts, and so checks, the whole tail;
    * a token with an underscore (``1_0``) is not an integer here; Python's ``int()`` accepts it.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _cabi
from ._engine import CabiEngine

INTS_STATUS_BITS = {
    _cabi.STATUS_TEXT_NOT_INTEGER: "a token is not an integer",
    _cabi.STATUS_TEXT_INT32_RANGE: "a kept token's value is outside int32",
    _cabi.STATUS_TEXT_SHORT: "the text holds fewer tokens than max_tokens",
    _cabi.STATUS_TEXT_LINE_SHAPE: "a record does not sit on a line of its own (line_records)",
}
HEAD_BYTES = 4096                                     # where the first line's newline is looked for
SEPARATORS = b"\t\n\x0b\x0c\r "


def padded(nbytes):
    """the capacity a text of ``nbytes`` needs: rounded up to 16, and 16 at least"""
    return max(16, (int(nbytes) + 15) // 16 * 16)


class TextIngestEngine(CabiEngine):
    """C-ABI calls of the text reader.  ``lib``/``ptr`` are injectable for the emulator tests only."""

    def __init__(self, lib=None, ptr=None, device="cuda:0"):
        super().__init__(lib, ptr, device)

    # ------------------------------------------------------------------ upload
    def upload(self, source, chunk_bytes=64 << 20):
        """a path, ``bytes`` or a uint8 array -> (text, nbytes): a uint8 tensor of ``padded(nbytes)`` bytes where the kernels run,
        zeros behind the text.  A file is read with ``readinto`` into two alternating staging buffers of ``chunk_bytes`` (pinned on
        the product path) and copied chunk by chunk: host memory stays at two chunks."""
        text, nbytes, _ = self._upload(source, chunk_bytes)
        return text, nbytes

    def _upload(self, source, chunk_bytes):
        """-> (text, nbytes, the first HEAD_BYTES bytes of the source)"""
        self.require_device(self.device)
        chunk_bytes = int(chunk_bytes)
        if chunk_bytes < 1:
            raise ValueError(f"chunk_bytes {chunk_bytes} must be positive")
        if isinstance(source, (str, os.PathLike)):
            return self._upload_file(os.fspath(source), chunk_bytes)
        data = np.frombuffer(source, dtype=np.uint8) if isinstance(source, (bytes, bytearray, memoryview)) else np.asarray(source)
        if data.dtype != np.uint8 or data.ndim != 1:
            raise ValueError("the text must be a path, bytes or a one-dimensional uint8 array")
        nbytes = int(data.size)
        text = self._empty_text(nbytes)
        if nbytes:
            text[:nbytes].copy_(torch.from_numpy(np.ascontiguousarray(data).copy()))
        return text, nbytes, data[:HEAD_BYTES].tobytes()

    def _empty_text(self, nbytes):
        text = torch.empty(padded(nbytes), dtype=torch.uint8, device=self.device)
        text[nbytes:].zero_()
        return text

    def _upload_file(self, path, chunk_bytes):
        pinned = self.device.type == "cuda"
        with open(path, "rb", buffering=0) as f:
            nbytes = os.fstat(f.fileno()).st_size
            text = self._empty_text(nbytes)
            stage = [torch.empty(min(chunk_bytes, max(nbytes, 1)), dtype=torch.uint8, pin_memory=pinned) for _ in range(2)]
            busy = [None, None]                       # the event after a staging buffer's last copy
            head, at, turn = b"", 0, 0
            while at < nbytes:
                buf = stage[turn]
                if busy[turn] is not None:
                    busy[turn].synchronize()          # (the copy two chunks ago: long done while the last one was read)
                want = min(buf.numel(), nbytes - at)
                view = memoryview(buf.numpy())[:want]
                got = 0
                while got < want:
                    k = f.readinto(view[got:])
                    if not k:
                        raise ValueError(f"{path}: the file shrank while it was read ({at + got} of {nbytes} bytes)")
                    got += k
                if at == 0:
                    head = bytes(view[:HEAD_BYTES])
                text[at:at + want].copy_(buf[:want], non_blocking=pinned)
                if pinned:
                    busy[turn] = torch.cuda.Event()
                    busy[turn].record(torch.cuda.current_stream(self.device))
                at += want
                turn ^= 1
            for ev in busy:
                if ev is not None:
                    ev.synchronize()                  # (the staging buffers are freed on return)
        return text, nbytes, head

    # ------------------------------------------------------------------ the bare calls
    def _check_text(self, text):
        if not isinstance(text, torch.Tensor) or text.dtype != torch.uint8 or text.dim() != 1 or not text.is_contiguous():
            raise ValueError("text must be a contiguous one-dimensional uint8 tensor (TextIngestEngine.upload makes one)")
        self.require_device(text)

    def line_ends(self, text, nbytes, lines, workspace_bytes=None):
        """-> int64 device tensor [len(lines) + 1]: the offset of the newline that ends each of the zero-based ``lines`` (-1 where
        the text has fewer lines), then the number of newlines in the text.  Nothing is read back."""
        self._check_text(text)
        lines = [int(x) for x in lines]
        arr = (ctypes.c_int64 * max(len(lines), 1))(*lines)
        a = _cabi.GccTextLineEndsArgs()
        a.text, a.nbytes, a.capacity = self.ptr(text), int(nbytes), int(text.numel())
        a.lines, a.num_lines = arr, len(lines)
        ends = torch.empty(min(len(lines), _cabi.TEXT_MAX_QUERIES) + 1, dtype=torch.int64, device=text.device)
        a.ends = self.ptr(ends)
        need = _cabi.size_query(self.lib, "gcc_text_line_ends_workspace_bytes", int(nbytes))
        status = torch.zeros(1, dtype=torch.int32, device=text.device)
        self.invoke("gcc_text_line_ends", a, self.workspace(need, text.device), status, workspace_bytes)
        return ends

    def ints_into(self, text, nbytes, first_byte, max_tokens, fields, keep, out, summary, status, workspace_bytes=None, capacity=None):
        """The bare call with the outputs as the caller allocated them (``out`` int32 of max_tokens / fields * keep words, ``summary``
        int64 [4], ``status`` zeroed int32 [1]).  Enqueued on torch's current stream; nothing is read back."""
        a = _cabi.GccTextIntsArgs()
        a.text = self.ptr(text) if text is not None else None
        a.nbytes, a.capacity = int(nbytes), int(text.numel() if capacity is None else capacity)
        a.first_byte, a.max_tokens, a.fields, a.keep = int(first_byte), int(max_tokens), int(fields), int(keep)
        a.out = self.ptr(out) if out is not None and out.numel() else None
        a.summary = self.ptr(summary) if summary is not None else None
        need = _cabi.size_query(self.lib, "gcc_text_ints_workspace_bytes", int(nbytes))
        self.invoke("gcc_text_ints", a, self.workspace(need, status.device), status, workspace_bytes)

    def ints(self, text, nbytes, first_byte, max_tokens, fields, keep):
        """-> dict(out int32 [max_tokens / fields, keep], summary int64 [4], status int32 [1]), all on the device; nothing is read
        back.  ``summary`` and ``status`` are two views of one buffer (``report``), so that one host read brings both."""
        self._check_text(text)
        max_tokens, fields, keep = int(max_tokens), int(fields), int(keep)
        records = max_tokens // fields if 1 <= fields <= 4 and max_tokens >= 0 and max_tokens % fields == 0 else 0
        words = records * keep if 1 <= keep <= fields and records * keep < 2 ** 31 else 0          # (the call refuses the rest by name)
        out = torch.empty((words // keep if words else 0, keep if words else max(keep, 1)), dtype=torch.int32, device=text.device)
        report = torch.zeros(5, dtype=torch.int64, device=text.device)
        summary, status = report[:4], report[4:].view(torch.int32)[:1]
        self.ints_into(text, nbytes, first_byte, max_tokens, fields, keep, out, summary, status)
        return dict(out=out, summary=summary, status=status, report=report)

    def ints_sep_into(self, text, nbytes, first_byte, max_tokens, fields, keep, out, summary, status, extra_sep=0, line_records=0,
                      workspace_bytes=None, capacity=None):
        """``ints_into`` through gcc_text_ints_sep: ``extra_sep`` is a seventh separator (0: none), ``line_records`` ties records to
        lines (``summary[3]``: the lowest offending token, or -1).  ``out`` may be None with ``max_tokens == 0``: the count-only call."""
        a = _cabi.GccTextIntsSepArgs()
        a.ints.text = self.ptr(text) if text is not None else None
        a.ints.nbytes, a.ints.capacity = int(nbytes), int(text.numel() if capacity is None else capacity)
        a.ints.first_byte, a.ints.max_tokens, a.ints.fields, a.ints.keep = int(first_byte), int(max_tokens), int(fields), int(keep)
        a.ints.out = self.ptr(out) if out is not None and out.numel() else None
        a.ints.summary = self.ptr(summary) if summary is not None else None
        a.extra_sep, a.line_records = int(extra_sep), int(line_records)
        need = _cabi.size_query(self.lib, "gcc_text_ints_workspace_bytes", int(nbytes))
        self.invoke("gcc_text_ints_sep", a, self.workspace(need, status.device), status, workspace_bytes)

    def ints_sep(self, text, nbytes, first_byte, max_tokens, fields, keep, extra_sep=0, line_records=0):
        """``ints`` with the two knobs of gcc_text_ints_sep -> the same dict"""
        self._check_text(text)
        max_tokens, fields, keep = int(max_tokens), int(fields), int(keep)
        records = max_tokens // fields if 1 <= fields <= 4 and max_tokens >= 0 and max_tokens % fields == 0 else 0
        words = records * keep if 1 <= keep <= fields and records * keep < 2 ** 31 else 0          # (the call refuses the rest by name)
        out = torch.empty((words // keep if words else 0, keep if words else max(keep, 1)), dtype=torch.int32, device=text.device)
        report = torch.zeros(5, dtype=torch.int64, device=text.device)
        summary, status = report[:4], report[4:].view(torch.int32)[:1]
        self.ints_sep_into(text, nbytes, first_byte, max_tokens, fields, keep, out, summary, status, extra_sep, line_records)
        return dict(out=out, summary=summary, status=status, report=report)

    @staticmethod
    def read_report(result):
        """one host read -> (summary as four ints, the status word)"""
        r = result["report"].cpu()
        return [int(x) for x in r[:4]], int(r[4:].view(torch.int32)[0])

    # ------------------------------------------------------------------ the .lscc layout
    def read_lscc(self, source, chunk_bytes=64 << 20):
        """``gcc_amd.ingest.read_lscc`` with the text on the device -> (n, pairs int32 device tensor [m, 2]).  ``source``: a path,
        ``bytes`` or a uint8 array.  Raises the host reader's ValueErrors (see the module docstring for the two differences)."""
        path = os.fspath(source) if isinstance(source, (str, os.PathLike)) else "<text>"
        text, nbytes, head = self._upload(source, chunk_bytes)

        def count_of(line, what):
            words = line.split()
            if len(words) < 2 or not words[1].lstrip(b"-").isdigit():
                raise ValueError(f"{path}: expected a `<word> {what}` line, found {line[:40]!r}")
            return int(words[1])

        first_end = head.find(b"\n")
        if first_end < 0:
            if nbytes <= HEAD_BYTES:
                raise ValueError(f"{path}: truncated: no `<word> n` line")
            raise ValueError(f"{path}: expected a `<word> n` line, found {head[:40]!r}")
        n = count_of(head[:first_end], "n")
        ends = [int(x) for x in self.line_ends(text, nbytes, [n, n + 1] if n >= 0 else []).cpu()]
        if n < 0 or ends[1] < 0:
            raise ValueError(f"{path}: truncated: {n} vertex lines and a `<word> m` line announced, the file has {ends[-1]} lines")
        m_line = text[ends[0] + 1:min(ends[1], ends[0] + 1 + HEAD_BYTES)].cpu().numpy().tobytes()
        m = count_of(m_line, "m")
        first = ends[1] + 1
        res = self.ints(text, nbytes, first, 3 * max(m, 0), 3, 2)
        (tokens, bad_at, range_at, _), status = self.read_report(res)
        if status & _cabi.STATUS_TEXT_NOT_INTEGER:
            token = text[bad_at:min(bad_at + 64, nbytes)].cpu().numpy().tobytes().split()[0]
            raise ValueError(f"{path}: an edge line holds something other than integers (the token {token[:40]!r} at byte {bad_at})")
        if m < 0 or status & _cabi.STATUS_TEXT_SHORT:
            raise ValueError(f"{path}: truncated: {m} edge lines `u v w` announced, {tokens // 3} complete ones found")
        if status & _cabi.STATUS_TEXT_INT32_RANGE:
            raise ValueError(f"{path}: node ids must fit int32")
        return n, res["out"]
