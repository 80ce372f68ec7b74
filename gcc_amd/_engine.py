"""What the engines of the downstream tasks and of the corpus build share (gcc_amd.logreg, svc, simsearch, prone, graphwave,
graph_build, graph_tables): the library and pointer
seam, the reused workspace, the checks on an embedding table, the C-ABI call and the status word.  A new task's engine derives
from CabiEngine; its C side starts from gcc_amd/csrc/task_common.h."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _cabi


class CabiEngine:
    """``lib``/``ptr`` are injectable for the emulator tests only; ``device``: where an engine that is handed arrays puts them."""

    def __init__(self, lib=None, ptr=None, device=None):
        self.lib = lib if lib is not None else _cabi.load()
        self.ptr = ptr if ptr is not None else _cabi.dev_ptr
        self.device = torch.device(device) if device is not None else None
        self._workspace = None

    def workspace(self, nbytes, device=None):
        """a buffer of at least ``nbytes`` that later calls reuse (stream-ordered: calls on ONE stream may share it), on
        ``device`` or the engine's own"""
        ws = self._workspace
        if ws is None or ws.numel() < nbytes or (device is not None and ws.device != device):
            self._workspace = None             # (the old one first: a corpus of 16,384 rows needs a GiB)
            ws = self._workspace = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device if device is not None else self.device)
        return ws

    def require_device(self, t):
        """the product path refuses a tensor (or a device) off the GPU by name; an injected ``ptr`` takes what it is given"""
        where = t.device if isinstance(t, torch.Tensor) else t
        if self.ptr is _cabi.dev_ptr and where.type != "cuda":
            raise RuntimeError("gcc_amd kernels take device (HIP) tensors only; there is no CPU path")

    def table(self, t, name="emb"):
        """-> (address, rows, D, row stride) of a float32 embedding table; a view with a row stride larger than D is passed as
        it is"""
        if t.dtype != torch.float32 or t.dim() != 2 or (t.numel() > 0 and t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError(f"{name} must be a float32 matrix with unit stride along its rows")
        self.require_device(t)
        rows, D = int(t.shape[0]), int(t.shape[1])
        return t.data_ptr(), rows, D, (int(t.stride(0)) if rows > 1 else D)

    def put(self, a, dtype):
        """a contiguous tensor of ``dtype`` where the kernels run; a tensor that is already one is passed as it is (the product
        path then refuses a CPU tensor by name)"""
        if isinstance(a, torch.Tensor):
            return a.to(dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(self.device).contiguous()

    def invoke(self, name, args, workspace, status, workspace_bytes=None, stream=None):
        """``name(args, workspace, its size or the one given, status, stream)``; ``stream`` defaults to torch's current one
        where the workspace lives"""
        _cabi.call(self.lib, name, ctypes.byref(args), self.ptr(workspace),
                   workspace.numel() if workspace_bytes is None else int(workspace_bytes), self.ptr(status),
                   _cabi.raw_stream(workspace.device) if stream is None else stream)

    @staticmethod
    def raise_status(result, prefix, bits_table, allow=0):
        """Raises and names the bits of the call's status word that ``allow`` does not cover (one host read)."""
        bits = int(result["status"].cpu()[0]) & ~allow
        if bits:
            raise RuntimeError(prefix + ": " + "; ".join(text for bit, text in bits_table.items() if bits & bit))
