"""gcc_amd._cabi.bind_batch -- the one place that turns a batch into the fields of an encoder call -- and the host batcher of the
whole-graph datasets, on CPU tensors: the capacity rule on a recording stub (no C symbol may be called for a refused batch), the
defaults of hand-built batches, the col_idx stand-in, and the emulator's output on the accepted batch."""
import numpy as np
import pytest
import torch

from gcc_amd import _cabi
from tests import batch_binding_check as C


class RecordingLib:
    """behind an engine's ``lib=``: records every symbol called and answers 0 (success; a size of 0 bytes)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0

        return fn


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _emu():
    from tests.hipemu.emu_driver import emu_lib

    return dict(lib=emu_lib(), ptr=_ptr)


@pytest.mark.parametrize("engine,field", C.CASES)
def test_short_array_is_refused_by_name_before_any_c_call(engine, field):
    lib = RecordingLib()
    C.refused(engine, C.encoder(engine), C.batch(short=field), field, lib=lib, ptr=_ptr)
    assert lib.calls == []


@pytest.mark.parametrize("engine", list(C.ENGINES))
def test_larger_position_table_is_accepted_and_the_capacity_unchanged(engine):
    lib = RecordingLib()
    C.call(engine, C.encoder(engine), C.batch(pos_rows=C.CAP + 5), lib=lib, ptr=_ptr)
    name, args = lib.calls[-1]
    assert name == C.ENGINES[engine][1]
    st = args[0]._obj if hasattr(args[0], "_obj") else args[0][0]       # byref(struct), or the array of passes
    assert st.node_cap == C.CAP and st.batch_size == 2


@pytest.mark.parametrize("engine", list(C.ENGINES))
def test_emulator_output_does_not_depend_on_rows_past_the_capacity(engine):
    enc = C.encoder(engine)
    a = C.call(engine, enc, C.batch(), **_emu()).clone()
    b = C.call(engine, enc, C.batch(pos_rows=C.CAP + 5), **_emu())
    assert tuple(a.shape)[0] == 2 and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    assert torch.equal(a, b)


def test_hand_built_batch_binds_with_the_defaults():
    g = C.batch()
    del g.parent_nid
    g.graph_id = torch.zeros(C.CAP + 2, dtype=torch.int32)              # without parent_nid: the capacity is graph_id's length
    g.row_ptr = torch.zeros(C.CAP + 3, dtype=torch.int32)
    g.pos_undirected = torch.zeros(C.CAP + 2, C.POS)
    assert not hasattr(g, "seed_local") and not hasattr(g, "edge_multiplicity")
    b = _cabi.bind_batch(g, _ptr, need_graph_id=True)
    assert b.seed_local is None and b.edge_multiplicity == 1 and b.node_cap == g.graph_id.numel() == C.CAP + 2
    assert (b.node_off, b.row_ptr, b.col_idx, b.graph_id, b.pos) == tuple(
        t.data_ptr() for t in (g.node_off, g.row_ptr, g.col_idx, g.graph_id, g.pos_undirected))
    assert b.batch_size == 2 and b.device == g.node_off.device and b.keep == ()
    with pytest.raises(AttributeError):
        b.node_cap = 1                                                  # the record is immutable
    g.seed_local, g.edge_multiplicity = torch.zeros(2, dtype=torch.int32), 2
    b = _cabi.bind_batch(g, _ptr)
    assert b.seed_local == g.seed_local.data_ptr() and b.edge_multiplicity == 2 and b.graph_id is None
    g.pos_undirected = None
    with pytest.raises(RuntimeError, match=r"^the batch has no pos_undirected \(run the positional embedding first\)$"):
        _cabi.bind_batch(g, _ptr)
    assert _cabi.bind_batch(g, _ptr, need_pos=False).pos is None


def test_batched_csr_constructor_states_every_field():
    from gcc_amd.sampler import BatchedCSR

    g = C.batch()
    b = BatchedCSR(2, g.node_off, g.edge_off, g.parent_nid, g.graph_id, g.row_ptr, g.col_idx)
    assert b.seed_local is None and b.valid == b.batch_size == 2 and b.edge_multiplicity == 1 and b.pos_undirected is None
    assert b.ndata["seed"].tolist() == [1, 0, 0, 1, 0]                  # seed_local None: the seed is local node 0
    for field in ("seed_local", "valid", "edge_multiplicity", "pos_undirected", "parent_nid", "graph_id"):
        assert field in BatchedCSR.__doc__, field


def test_col_idx_stand_in_only_where_asked_for():
    g = C.batch()
    g.col_idx = torch.zeros(0, dtype=torch.int32)
    assert _ptr(g.col_idx) == 0
    b = _cabi.bind_batch(g, _ptr, col_placeholder=True)
    (stand_in,) = b.keep
    assert b.col_idx == stand_in.data_ptr() != 0
    assert tuple(stand_in.shape) == (1,) and stand_in.dtype == torch.int32 and stand_in.device == g.node_off.device
    assert _cabi.bind_batch(g, _ptr).col_idx == _ptr(g.col_idx)         # not asked for: what ptr gives
    full = C.batch()
    b = _cabi.bind_batch(full, _ptr, col_placeholder=True)
    assert b.col_idx == full.col_idx.data_ptr() and b.keep == ()        # live entries: no stand-in


# ------------------------------------------------------------------------------------------------ the host batcher
GRAPHS = [(np.array([0, 2, 4, 6]), np.array([1, 2, 0, 2, 0, 1])),      # a triangle
          (np.array([0, 0]), np.array([], dtype=np.int64)),              # one isolated node
          (np.array([0, 1, 2]), np.array([1, 0]))]                       # a path of two nodes


def _host_dataset():
    from gcc_amd.datasets import GraphClassificationDataset

    ds = GraphClassificationDataset(graphs=GRAPHS, batch_size=4, device="cpu")
    assert ds.batcher == "host" and ds.node_cap == 16
    return ds


def test_host_batcher_on_three_graphs():
    ds = _host_dataset()
    for g in (ds._batch_of([0, 1, 2]), next(iter(ds))[0]):              # iteration runs the same batcher
        assert g.node_off.tolist() == [0, 3, 4, 6, 6]
        assert g.edge_off.tolist() == [0, 6, 6, 8, 8]
        assert g.row_ptr[:7].tolist() == [0, 2, 4, 6, 6, 7, 8] and g.row_ptr.numel() == 17
        assert g.graph_id.tolist() == [0, 0, 0, 1, 2, 2] + [0] * 10
        assert g.col_idx.tolist() == [1, 2, 0, 2, 0, 1, 5, 4]
        assert g.seed_local.tolist() == [0, 0, 0, 0]
        assert g.valid == 3 and g.batch_size == 4 and g.parent_nid.numel() == 16
        assert all(t.dtype == torch.int32 for t in (g.node_off, g.edge_off, g.row_ptr, g.graph_id, g.col_idx, g.seed_local))


def test_host_batcher_on_an_edge_free_batch():
    g = _host_dataset()._batch_of([1])
    assert g.node_off.tolist() == [0, 1, 1, 1, 1]
    assert g.edge_off.tolist() == [0, 0, 0, 0, 0]
    assert g.row_ptr[:2].tolist() == [0, 0]
    assert g.graph_id.tolist() == [0] * 16
    assert g.col_idx.tolist() == [0]                                    # one element: never read, but its address is not null
    assert g.seed_local.tolist() == [0, 0, 0, 0]
    assert g.valid == 1
