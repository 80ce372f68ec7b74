"""Wide (hidden 256) GIN layers in bf16 on the matrix cores: the host side of ``gcc_ginw_forward``
(include/gcc_amd.h), BASELINE.json configs[4].

``FoldedWideGIN`` holds the layer stack of UnsupervisedGIN (gcc/models/gin.py:160-221) for inference
(generate.py:71 ``model.eval()``): Linear weights as bf16, Linear biases and BatchNorm running statistics folded
into per-channel scale/shift pairs.  Device only: there is no CPU path.

``WideResidentEngine`` is the host side of ``gcc_ginw_embed``: the eval-mode embedding of a wide ``GraphEncoder``
(``GraphEncoder.resident_eval``, ``generate.py --wide-eval resident``) on those layers, from feature assembly to the
mean of the two views, in one call.
"""
from __future__ import annotations

import ctypes

import torch

from . import _cabi

HIDDEN = 256
MAX_NODES = 128


def fold_bn(bn, bias=None):
    """(scale, shift) of eval-mode BatchNorm1d applied to ``x + bias``."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    b = torch.zeros_like(s) if bias is None else bias.detach().double()
    return s.float(), ((b - bn.running_mean.detach().double()) * s + bn.bias.detach().double()).float()


class FoldedWideGIN:
    def __init__(self, layers, device, lib=None, ptr=None):
        """layers: list of dicts with float32 tensors w0, w1 [256, 256] (torch Linear layout) and s0..t2 [256].
        ``lib`` / ``ptr`` are injectable only so that the tests can run the same host code against the emulator build."""
        self.device = torch.device(device)
        if lib is None and self.device.type != "cuda":
            raise RuntimeError("gcc_amd kernels run on the GPU only; there is no CPU path")
        if not 1 <= len(layers) <= 8:
            raise ValueError("1 to 8 layers")
        self.lib = lib if lib is not None else _cabi.load()
        self.ptr = ptr if ptr is not None else _cabi.dev_ptr
        self.layers = []
        for ly in layers:
            d = {}
            for k in ("w0", "w1"):
                w = torch.as_tensor(ly[k], dtype=torch.float32)
                if tuple(w.shape) != (HIDDEN, HIDDEN):
                    raise ValueError(f"{k} must be [{HIDDEN}, {HIDDEN}]")
                d[k] = w.to(self.device).to(torch.bfloat16).contiguous()          # round to nearest even
            for k in ("s0", "t0", "s1", "t1", "s2", "t2"):
                v = torch.as_tensor(ly[k], dtype=torch.float32)
                if tuple(v.shape) != (HIDDEN,):
                    raise ValueError(f"{k} must be [{HIDDEN}]")
                d[k] = v.to(self.device).contiguous()
            # the same weights in the order the kernel's waves request them (include/gcc_amd.h: gcc_ginw_pack_weights)
            st = _cabi.raw_stream(self.device)
            for which, k in enumerate(("w0", "w1")):
                d[k + "_frag"] = torch.empty_like(d[k])
                _cabi.call(self.lib, "gcc_ginw_pack_weights", self.ptr(d[k]), self.ptr(d[k + "_frag"]), which, st)
            self.layers.append(d)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._scratch = None             # rows in transit + work list of subgraphs over 128 nodes (gcc_ginw_scratch_bytes)

    @classmethod
    def from_gin(cls, gin, device):
        """gin: a module with the reference's attribute names (``ginlayers[i].apply_func.{mlp,bn}``,
        ``batch_norms[i]``; gin.py:160-199) whose hidden size is 256."""
        layers = []
        for i, layer in enumerate(gin.ginlayers):
            mlp = layer.apply_func.mlp
            s0, t0 = fold_bn(mlp.batch_norms[0], mlp.linears[0].bias)
            s1, t1 = fold_bn(layer.apply_func.bn, mlp.linears[1].bias)
            s2, t2 = fold_bn(gin.batch_norms[i])
            layers.append(dict(w0=mlp.linears[0].weight.detach(), w1=mlp.linears[1].weight.detach(),
                               s0=s0, t0=t0, s1=s1, t1=t1, s2=s2, t2=t2))
        return cls(layers, device)

    @classmethod
    def from_encoder(cls, enc, lib=None, ptr=None):
        """The layer stack of a wide GIN ``GraphEncoder`` (input, hidden and output widths up to 256), zero-padded to 256
        channels: layer 0's [hidden, d_in] weight sits in the top left corner of its [256, 256] block, every other weight is
        a [hidden, hidden] corner, scales and shifts end in zeros.  A padded channel has scale 0 and shift 0, so it is
        relu(0 * x + 0) = 0 after every BatchNorm and meets only zero weights: the padded model is the model (DESIGN.md
        section 4d makes the same argument for widths below 64).  The prediction layers are not folded: the readout reads
        the encoder's own f32 tensors."""
        layers = []
        dev = enc.degree_embedding.weight.device

        def corner(w):
            out = torch.zeros(HIDDEN, HIDDEN, dtype=torch.float32, device=w.device)
            out[: w.shape[0], : w.shape[1]] = w.detach()
            return out

        def head(v):
            out = torch.zeros(HIDDEN, dtype=torch.float32, device=v.device)
            out[: v.shape[0]] = v
            return out

        for i, layer in enumerate(enc.gnn.ginlayers):
            mlp = layer.apply_func.mlp
            s0, t0 = fold_bn(mlp.batch_norms[0], mlp.linears[0].bias)
            s1, t1 = fold_bn(layer.apply_func.bn, mlp.linears[1].bias)
            s2, t2 = fold_bn(enc.gnn.batch_norms[i])
            layers.append(dict(w0=corner(mlp.linears[0].weight), w1=corner(mlp.linears[1].weight), s0=head(s0), t0=head(t0),
                               s1=head(s1), t1=head(t1), s2=head(s2), t2=head(t2)))
        return cls(layers, dev, lib=lib, ptr=ptr)

    def forward(self, node_off, row_ptr, col_idx, x, num_layers=None, first_layer=0, want_rows=True, want_pooled=True,
                prof=None, big=True):
        """x: bf16 [N, 256] on the device; the CSR is the batched graph of the sampler (int32, row v = in-neighbours
        of v, global ids).  Runs layers first_layer .. first_layer + num_layers - 1 in one launch.  Returns (rows bf16 [N, 256] or None, pooled f32 [B, L + 1, 256] or None); call
        ``check_status()`` after synchronising."""
        L = len(self.layers) - first_layer if num_layers is None else int(num_layers)
        if not (0 <= first_layer and 1 <= L and first_layer + L <= len(self.layers)):
            raise ValueError("layer range out of bounds")
        if x.dtype != torch.bfloat16 or x.dim() != 2 or x.shape[1] != HIDDEN:
            raise TypeError(f"x must be bfloat16 [N, {HIDDEN}]")
        B = node_off.numel() - 1
        rows = torch.empty_like(x) if want_rows else None
        pooled = torch.empty(B, L + 1, HIDDEN, dtype=torch.float32, device=self.device) if want_pooled else None
        a = _cabi.GccGinwArgs(node_off=_cabi.dev_ptr(node_off, torch.int32), row_ptr=_cabi.dev_ptr(row_ptr, torch.int32),
                              col_idx=_cabi.dev_ptr(col_idx, torch.int32), x_in=_cabi.dev_ptr(x),
                              x_out=_cabi.dev_ptr(rows), pooled=_cabi.dev_ptr(pooled), batch_size=B, num_layers=L)
        for i in range(L):
            for k, v in self.layers[first_layer + i].items():
                setattr(a.layers[i], k, _cabi.dev_ptr(v))
        if big:
            # subgraphs over 128 nodes run block by block (one launch per layer for them); without the scratch they are
            # refused through the status word
            need = int(self.lib.gcc_ginw_scratch_bytes(x.shape[0], B))
            if self._scratch is None or self._scratch.numel() < need:
                self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
            a.scratch, a.scratch_bytes, a.num_nodes = _cabi.dev_ptr(self._scratch), need, x.shape[0]
        st = _cabi.raw_stream(self.device)
        _cabi.call(self.lib, "gcc_ginw_forward", ctypes.byref(a), _cabi.dev_ptr(self.status),
                   prof.handle if prof is not None else None, st)
        return rows, pooled

    def check_status(self):
        s = int(self.status[0].item())
        if s & 32:
            raise RuntimeError(f"gcc_ginw_forward: a subgraph has more than {MAX_NODES} nodes and the call had no scratch "
                               "(big=False), or more row blocks than the work list holds: its outputs are zero")
        if s & 64:
            raise RuntimeError("gcc_ginw_forward: a neighbour id lies outside its subgraph")
        return s


STATUS_NAMES = (
    (_cabi.STATUS_GINW_TOO_LARGE, "a subgraph has more row blocks than the work list holds: its outputs are zero"),
    (_cabi.STATUS_GINW_BAD_EDGE, "a neighbour id lies outside its subgraph"),
    (_cabi.STATUS_GINW_COUNT_OVERFLOW, "a neighbour occurs more than 256 times in one row (CSR copies x edge multiplicity): the count "
                                       "has no exact bf16 value and the subgraph's embedding is wrong"),
)


def state_key(enc):
    """(address, version) of every parameter and buffer: changes when a tensor is replaced (``.to()``, ``.data = ``) or
    written in place (``load_state_dict``, an optimizer step)."""
    return tuple((t.data_ptr(), t._version) for t in list(enc.parameters()) + list(enc.buffers()))


class WideResidentEngine:
    """Fold cache, buffers and the C-ABI call of ``gcc_ginw_embed``.  ``lib`` / ``ptr`` are injectable only so that the
    tests can run the same host code against the emulator build."""

    def __init__(self, lib=None, ptr=None):
        self._inject = (lib, ptr)
        self.lib = lib if lib is not None else _cabi.load()
        self.ptr = ptr if ptr is not None else _cabi.dev_ptr
        self._fold = None                 # (state_key, FoldedWideGIN)
        self._bufs = {}
        self.status = None
        self.pooled = None                # [views, B, L + 1, 256] of the last call (the readout's input; tests read it)

    @staticmethod
    def refuse(enc):
        """NotImplementedError, by name, for every model this path does not serve."""
        if enc.gnn_model == "gat":
            raise NotImplementedError("resident_eval: the LDS-resident eval path serves GIN encoders; this one is a GAT (csrc/gat.hip "
                                      "has no resident kernel)")
        if not enc.wide:
            raise NotImplementedError(f"resident_eval: this model ({enc.hidden} / {enc.output_dim}) is not a wide GIN encoder; its eval path "
                                      "is gcc_gin_eval_fused (GraphEncoder.fused_eval), which is one launch already")
        d_in = enc.positional_embedding_size + enc.degree_embedding_size + 1
        if enc.hidden > HIDDEN or enc.output_dim > HIDDEN or d_in > HIDDEN:
            raise NotImplementedError(f"resident_eval: input / hidden / output widths up to {HIDDEN} are served (csrc/gin_wide.hip keeps "
                                      f"{HIDDEN} channels per node in LDS); this model has {d_in} / {enc.hidden} / {enc.output_dim}")
        if len(enc.gnn.ginlayers) > _cabi.GIN_MAX_LAYERS:
            raise NotImplementedError(f"resident_eval: at most {_cabi.GIN_MAX_LAYERS} GIN layers (this model has "
                                      f"{len(enc.gnn.ginlayers)})")
        if enc.training or any(m.training for m in enc.modules() if isinstance(m, torch.nn.BatchNorm1d)):
            raise NotImplementedError("resident_eval: training-mode BatchNorm (batch statistics; dropout with it) cannot be folded into "
                                      "the resident kernel's per-channel scale / shift; call model.eval() first (generate.py:38)")

    def folded(self, enc):
        key = state_key(enc)
        if self._fold is None or self._fold[0] != key:
            self._fold = (key, FoldedWideGIN.from_encoder(enc, *self._inject))
        return self._fold[1]

    def embed(self, enc, views):
        """views: one or two batches (BatchedCSR with pos_undirected) of the same batch size.  -> [B, output_dim] f32."""
        self.refuse(enc)
        ptr = self.ptr
        bound = [_cabi.bind_batch(g, ptr, col_placeholder=True) for g in views]      # (an edge-free batch: the C side refuses a null col_idx)
        b0 = bound[0]
        if any(b.batch_size != b0.batch_size or b.edge_multiplicity != b0.edge_multiplicity for b in bound):
            raise ValueError("the views of one call share batch size and edge multiplicity")
        fold = self.folded(enc)
        B, L, dev = b0.batch_size, len(fold.layers), b0.device
        node_cap = max(b.node_cap for b in bound)
        nbytes = _cabi.size_query(self.lib, "gcc_ginw_embed_workspace_bytes", node_cap, B)
        key = (nbytes, B, L, enc.output_dim, str(dev))
        if key not in self._bufs:
            self._bufs = {key: dict(ws=torch.empty(nbytes, dtype=torch.uint8, device=dev),
                                    pooled=torch.empty(2, B, L + 1, HIDDEN, dtype=torch.float32, device=dev),
                                    out=torch.empty(B, enc.output_dim, dtype=torch.float32, device=dev))}
        buf = self._bufs[key]
        if self.status is None or self.status.device != dev:
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        a = _cabi.GccGinwEmbedArgs(num_views=len(views), batch_size=B, num_layers=L, pos_dim=enc.positional_embedding_size,
                                   deg_emb_dim=enc.degree_embedding_size, max_degree=enc.max_degree,
                                   edge_multiplicity=max(b0.edge_multiplicity, 1), hidden=enc.hidden,
                                   out_dim=enc.output_dim, normalize=int(enc.norm), norm_eps=1e-5, node_cap=node_cap)   # graph_encoder.py:196
        for v, b in enumerate(bound):
            a.node_off[v], a.row_ptr[v], a.col_idx[v], a.seed_local[v], a.pos[v] = b.node_off, b.row_ptr, b.col_idx, b.seed_local, b.pos
            a.pooled[v] = ptr(buf["pooled"][v])
        a.degree_embedding = ptr(enc.degree_embedding.weight.detach())
        for i, ly in enumerate(fold.layers):
            for k, t in ly.items():
                setattr(a.layers[i], k, ptr(t))
        for i, lin in enumerate(enc.gnn.linears_prediction):
            a.pred_w[i], a.pred_b[i] = ptr(lin.weight.detach()), ptr(lin.bias.detach())
        a.out, a.workspace, a.workspace_bytes = ptr(buf["out"]), ptr(buf["ws"]), nbytes
        _cabi.call(self.lib, "gcc_ginw_embed", ctypes.byref(a), ptr(self.status), _cabi.raw_stream(dev))
        self.pooled = buf["pooled"][: len(views)]
        return buf["out"].clone()

    def check_status(self):
        """Raises, by name, for every status bit the calls so far have set (one host read); clears the word."""
        if self.status is None:
            return 0
        s = int(self.status[0].item())
        self.status.zero_()
        bad = [text for bit, text in STATUS_NAMES if s & bit]
        if bad:
            raise RuntimeError("gcc_ginw_embed: " + "; ".join(bad))
        return s
