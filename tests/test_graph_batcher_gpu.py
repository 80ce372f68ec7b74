"""gcc_pack_graphs on a real MI355X against the host batcher, exactly: the shapes of tests/graph_batcher_check.py through the C
ABI, the two dataset classes with ``batcher="device"`` against ``batcher="host"``, and the buffer ring under LabeledProducer's
prefetch."""
import numpy as np
import pytest
import torch

from tests import graph_batcher_check as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pack():
    from gcc_amd import _cabi

    return C.Packer(_cabi.load(), _cabi.dev_ptr, "cuda:0")


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


# ------------------------------------------------------------------------------------------------ the dataset classes
def _graphs(sizes, seed):
    return [C.ring_with_chords(n, seed + i) for i, n in enumerate(sizes)]


def _fields(g, lab=None):
    """everything a consumer reads of a batch, as host copies (a copy also pins down what the ring slot held at this moment)"""
    n = int(g.node_off[g.batch_size])
    out = dict(node_off=g.node_off, edge_off=g.edge_off, row_ptr=g.row_ptr[: n + 1], col_idx=g.col_idx, graph_id=g.graph_id[:n],
               seed_local=g.seed_local)
    if g.pos_undirected is not None:
        out["pos"] = g.pos_undirected[:n].view(torch.int32)
    if lab is not None:
        out["labels"] = lab
    out = {k: v.cpu().clone() for k, v in out.items()}
    out["valid"], out["edge_multiplicity"] = g.valid, g.edge_multiplicity
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def _labelled_pair(graphs, labels, B, mult, P=32):
    from gcc_amd.datasets import GraphClassificationDatasetLabeled

    pair = [GraphClassificationDatasetLabeled(graphs=graphs, labels=labels, positional_embedding_size=P, edge_multiplicity=mult,
                                              batch_size=B, device="cuda:0", batcher=b) for b in ("device", "host")]
    table = C.pos_table(int(pair[0].first[-1]), P).cuda()
    for ds in pair:
        ds._pos = table                                        # the same injected table on both sides: no eigensolver here
    return pair


@pytest.mark.parametrize("mult", [1, 2])
def test_labelled_dataset_device_batches_equal_host_batches(mult):
    graphs = _graphs((9, 24, 61, 15, 150, 33, 420), 40)
    dev, host = _labelled_pair(graphs, [0, 1, 2, 0, 1, 2, 0], 4, mult)
    assert dev.batcher == "device" and host.batcher == "host"
    order = np.random.RandomState(3).permutation(7)
    got = [_fields(g, y) for g, y in dev.batches(order)]
    ref = [_fields(g, y) for g, y in host.batches(order)]
    assert len(got) == len(ref) == 2 and got[1]["valid"] == 3              # the last batch is partial
    for a, b in zip(got, ref):
        _assert_same(a, b)
    a, b = _fields(*dev.make_batch([6, 6, 0])), _fields(*host.make_batch([6, 6, 0]))   # indices passed by the caller
    _assert_same(a, b)
    dev.check_status()


def test_unlabelled_dataset_device_batches_equal_host_batches():
    from gcc_amd.datasets import GraphClassificationDataset

    graphs = _graphs((9, 24, 61, 15, 150, 33, 420), 40)
    dev, host = [GraphClassificationDataset("toy", graphs=graphs, edge_multiplicity=2, batch_size=4, device="cuda:0", batcher=b)
                 for b in ("device", "host")]
    n = 0
    for (q, k), (hq, hk) in zip(dev, host):
        assert q is k and hq is hk
        _assert_same(_fields(q), _fields(hq))
        n += 1
    assert n == 2
    dev.check_status()
    auto = GraphClassificationDataset("toy", graphs=graphs, batch_size=4, device="cuda:0")
    assert auto.batcher == "device"                            # what "auto" means on a GPU


def test_ring_slots_survive_the_producer_prefetch():
    """LabeledProducer keeps depth + 1 batches in flight on its side stream; a batch cloned when it is handed out must be what
    the host batcher gives for the same indices -- three epochs of random orders, so every ring slot is reused many times"""
    from gcc_amd.finetune import LabeledProducer

    rng = np.random.RandomState(9)
    graphs = _graphs([int(x) for x in rng.randint(3, 300, 40)], 70)
    dev, host = _labelled_pair(graphs, [int(x) for x in rng.randint(0, 3, 40)], 8, 2, P=6)
    prod = LabeledProducer(dev, "cuda:0", prefetch=True, depth=1)
    for _ in range(3):
        order = rng.permutation(40)[:37]
        got = [_fields(g, y) for g, y in prod.batches(order)]
        assert len(got) == 5
        for i, a in enumerate(got):
            _assert_same(a, _fields(*host.make_batch(order[8 * i: 8 * i + 8])))
    dev.check_status()
