"""gcc_pack_graphs (gcc_amd/csrc/graph_batch.hip) on the lock-step emulator against the host batcher, exactly: the shapes of
tests/graph_batcher_check.py at both multiplicities and three positional sizes (16-byte lanes, 8-byte lanes, one lane per row),
the capacity cuts, the index rules -- and the ``batcher`` argument of the dataset classes off the GPU."""
import numpy as np
import pytest
import torch

from tests import graph_batcher_check as C
from tests.hipemu.emu_driver import emu_lib


@pytest.fixture(scope="module")
def pack():
    return C.Packer(emu_lib(), lambda t: t.data_ptr() if t is not None else None, "cpu")


@pytest.mark.parametrize("P", [32, 6, 2])
@pytest.mark.parametrize("expand", [1, 3])
@pytest.mark.parametrize("name", list(C.SHAPE_BATCHES))
def test_batch_equals_the_host_batcher(pack, name, expand, P):
    C.check_shape(pack, name, expand, P)


@pytest.mark.parametrize("P", [32, 6])
@pytest.mark.parametrize("expand", [1, 3])
@pytest.mark.parametrize("which", ["node", "edge"])
def test_capacity_overflow_cuts_at_a_graph_boundary(pack, which, expand, P):
    C.check_overflow(pack, which, expand, P)


def test_out_of_range_index_is_padding_with_a_status_bit(pack):
    C.check_bad_index(pack, 6)


def test_bad_arguments_are_refused_by_name(pack):
    C.check_refusals(pack)


def test_corpus_ring_hands_out_host_shaped_batches(pack):
    """DeviceGraphCorpus.pack on the emulator: col_idx is a view of exactly the live length (the one-element placeholder for an
    edge-free batch), the ring slots rotate, and the batch equals the host's"""
    from gcc_amd.datasets import DeviceGraphCorpus

    graphs, labels = C.shape_corpus()
    P, B, expand = 6, 4, 3
    c = DeviceGraphCorpus(graphs, B, labels=labels, pos_dim=P, expand=expand, device="cpu", num_buffers=2, lib=pack.lib,
                          ptr=pack.ptr)
    c.set_pos(C.pos_table(int(c.first[-1]), P))
    seen = []
    for idx in ([5, 2], [0], [3, 3, 8, 1]):
        ref = C.host_reference(B, expand, P, idx + [-1] * (B - len(idx)))
        g, lab = c.pack(c.index_tensor(idx), c.entries[idx].sum())
        assert g.col_idx.shape == (max(ref["e"], expand),) and g.parent_nid.shape == (c.node_cap,)
        if ref["e"] == 0:
            assert g.col_idx.tolist() == [0] * expand         # the host's one-element placeholder, repeated like every entry
        got = dict(node_off=g.node_off.numpy(), edge_off=g.edge_off.numpy(), graph_id=g.graph_id.numpy(),
                   row_ptr=g.row_ptr.numpy(), col_idx=g.col_idx.numpy(), seed_local=g.seed_local.numpy(), labels=lab.numpy(),
                   pos=g.pos_undirected.numpy().view(np.int32).reshape(-1))
        C.assert_equals_host(got, ref, B, P)
        seen.append(g.node_off.data_ptr())
    assert seen[0] == seen[2] != seen[1]
    c.check_status()
    c.pack(torch.tensor([2, 50, -1, -1], dtype=torch.int32), c.entries[[2]].sum())
    with pytest.raises(RuntimeError, match="graph index out of range"):
        c.check_status()


def test_device_batcher_off_the_gpu_is_refused_by_name_and_auto_is_the_host_code():
    from gcc_amd.datasets import GraphClassificationDataset, GraphClassificationDatasetLabeled

    graphs, labels = C.shape_corpus()
    for cls, kw in ((GraphClassificationDataset, {}), (GraphClassificationDatasetLabeled, dict(labels=labels))):
        with pytest.raises(ValueError, match='batcher="device" needs a GPU device'):
            cls(graphs=graphs, batch_size=4, device="cpu", batcher="device", **kw)
        with pytest.raises(ValueError, match="batcher must be"):
            cls(graphs=graphs, batch_size=4, device="cpu", batcher="gpu", **kw)
        ds = cls(graphs=graphs, batch_size=4, device="cpu", **kw)
        assert ds.batcher == "host"
    ds = GraphClassificationDataset(graphs=graphs, batch_size=4, device="cpu")
    q, k = next(iter(ds))
    assert q is k and ds._corpus is None and q.valid == 4     # the NumPy loop: no corpus was uploaded
    ds.check_status()
