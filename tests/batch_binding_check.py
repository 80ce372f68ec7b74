"""Shared by tests/test_batch_binding_emu.py and tests/test_batch_binding_gpu.py: the two-graph batch of the capacity rule's tests
(gcc_amd._cabi.bind_batch) and one eval-mode call per encoder engine on it.  TEST INFRASTRUCTURE ONLY."""
from types import SimpleNamespace

import torch

from gcc_amd import _cabi
from gcc_amd.encoder import GatEngine, GinEngine, GraphEncoder
from gcc_amd.encoder_wide import WideGinEngine
from gcc_amd.gin_wide import WideResidentEngine

CAP, LIVE, POS = 9, 5, 32
# engine -> (the capacity-ruled fields it takes, the C call that receives the batch)
ENGINES = {"gin": (("row_ptr", "graph_id", "pos_undirected"), "gcc_gin_forward"),
           "wide": (("row_ptr", "graph_id", "pos_undirected"), "gcc_ginx_forward"),
           "gat": (("row_ptr", "pos_undirected"), "gcc_gat_forward"),
           "resident": (("row_ptr", "pos_undirected"), "gcc_ginw_embed")}
REQUIRED = {"row_ptr": CAP + 1, "graph_id": CAP, "pos_undirected": CAP}
CASES = [(e, f) for e, (fields, _) in ENGINES.items() for f in fields]


def batch(device="cpu", short=None, pos_rows=CAP):
    """A triangle and a path of two nodes -- node counts [3, 2] -- inside a capacity of 9 rows.  ``short``: that field one row
    too short for the capacity.  ``pos_rows``: rows of the position table (the live rows are the same for every size)."""
    i32 = dict(dtype=torch.int32)
    row_ptr = torch.zeros(CAP + 1, **i32)
    row_ptr[: LIVE + 1] = torch.tensor([0, 2, 4, 6, 7, 8], **i32)
    graph_id = torch.zeros(CAP, **i32)
    graph_id[:LIVE] = torch.tensor([0, 0, 0, 1, 1], **i32)
    pos = torch.nn.functional.normalize(torch.randn(CAP + 5, POS, generator=torch.Generator().manual_seed(7)), dim=1)
    g = SimpleNamespace(batch_size=2, node_off=torch.tensor([0, 3, 5], **i32), edge_off=torch.tensor([0, 6, 8], **i32),
                        parent_nid=torch.zeros(CAP, **i32), graph_id=graph_id, row_ptr=row_ptr,
                        col_idx=torch.tensor([1, 2, 0, 2, 0, 1, 4, 3], **i32), pos_undirected=pos[:pos_rows].contiguous())
    if short is not None:
        setattr(g, short, getattr(g, short)[:-1].contiguous())
        assert getattr(g, short).shape[0] == REQUIRED[short] - 1
    for name, t in vars(g).items():
        if isinstance(t, torch.Tensor):
            setattr(g, name, t.to(device))
    return g


def encoder(engine):
    """a small eval-mode encoder for ``engine``, the same weights on every call"""
    kw = dict(positional_embedding_size=POS, max_node_freq=16, max_edge_freq=16, max_degree=64, freq_embedding_size=16,
              degree_embedding_size=16, edge_hidden_dim=32, norm=True, degree_input=True)
    torch.manual_seed(11)
    if engine == "gat":
        enc = GraphEncoder(output_dim=32, node_hidden_dim=32, num_layers=2, num_heads=2, num_step_set2set=2, num_layer_set2set=1,
                           gnn_model="gat", **kw)
    else:
        width = 64 if engine == "gin" else 72
        enc = GraphEncoder(output_dim=width, node_hidden_dim=width, num_layers=3, gnn_model="gin", **kw)
        assert enc.wide == (engine != "gin")
    return enc.eval()


def call(engine, enc, g, **kw):
    """the engine's call on ``g`` in eval mode -> its [2, out] output.  ``kw``: ``lib=`` / ``ptr=`` of the emulator or of a stub;
    nothing on the device"""
    st = _cabi.raw_stream(g.node_off)
    if engine == "gin":
        eng = GinEngine(**kw)
        p, buf = eng.make_pass(enc, g, training=False)
        eng.forward([p], stream=st)
        return buf["feat"]
    if engine == "wide":
        eng = WideGinEngine(**kw)
        p, buf = eng.make_pass(enc, g, training=False)
        eng.forward(p, stream=st)
        return buf["feat"]
    if engine == "gat":
        return GatEngine(**kw).forward(enc, g, stream=st)[0]
    return WideResidentEngine(**kw).embed(enc, [g])


def refused(engine, enc, g, field, **kw):
    """the call on a batch whose ``field`` is one row short raises RuntimeError with the field, its size and the required size"""
    import pytest

    need = REQUIRED[field]
    with pytest.raises(RuntimeError, match=rf"{field} has {need - 1} rows.* needs at least {need}\b"):
        call(engine, enc, g, **kw)
