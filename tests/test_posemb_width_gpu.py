"""The positional-embedding solver at widths 2 .. 32, into pre-filled output buffers, on disconnected graphs and isolated nodes
-- on a real MI355X (cases, checker and bars: tests/posemb_width_check.py).  Every item of a width in ONE call per knob setting:
the k edge, the one-wave teams, the four-wave / 1,024-thread 65..128 class, the block and slot classes, the 385..704 class and
Krylov; check_status(strict=True)."""
import numpy as np
import pytest
import torch

from tests import posemb_width_check as W

pytestmark = pytest.mark.gpu


def _batch(view, cap, hid):
    from gcc_amd.sampler import BatchedCSR

    no, rp, ci = (view[k].numpy() for k in ("node_off", "row_ptr", "col_idx"))
    B, n = len(no) - 1, int(no[-1])
    rows = np.full(cap + 1, rp[-1], dtype=np.int32)                  # (the rows beyond N are empty)
    rows[:n + 1] = rp
    gid = np.zeros(cap, dtype=np.int32)
    gid[:n] = np.repeat(np.arange(B), np.diff(no))
    return BatchedCSR(B, torch.from_numpy(no.astype(np.int32)).cuda(), torch.from_numpy(rp[no].astype(np.int32)).cuda(),
                      torch.zeros(cap, dtype=torch.int32, device="cuda"), torch.from_numpy(gid).cuda(),
                      torch.from_numpy(rows).cuda(), torch.from_numpy(ci.astype(np.int32)).cuda())


def _pe(B, cap, hid):
    from gcc_amd.posemb import DevicePosEmb

    return DevicePosEmb(B, cap, hid, device="cuda", seed=7, num_buffers=1)


@pytest.mark.parametrize("knob", list(W.KNOBS))
@pytest.mark.parametrize("hid", W.WIDTHS)
def test_every_item_in_one_call(hid, knob):
    names, view = W.batch(W.width_items(hid, heavy=True))
    assert int(np.diff(view["node_off"].numpy()).max()) <= 1200
    with W.Knobs(knob):
        x, evals, raw, status = W.run_filled(view, hid, _batch, _pe)
    cls = set(W.expected_status(names, view, knob, status))
    assert cls == {"default": {"zeros", "w48", "w64", "pair", "block"},
                   "wave0": {"zeros", "small", "pair", "block"},
                   "pair0": {"zeros", "w48", "w64", "mid", "block"},
                   "cheb0": {"zeros", "w48", "w64", "pair", "slot", "big", "krylov"}}[knob], cls
    W.check_batch(names, view, hid, x, evals, raw)


def test_a_smaller_batch_in_a_ring_slot_that_held_a_larger_one():
    """Width 30, num_buffers=1, no sentinel: the production shape of a stale output buffer.  The large batch passes through both
    ring slots, then the small one lands in the first: its rows and padding columns are what a fresh DevicePosEmb writes, bit
    for bit, and meet the invariants; nothing of the large batch's embedding is in them."""
    hid = 30
    big_names, big = W.batch(W.width_items(hid, heavy=True))
    names, small = W.batch(W.width_items(hid, only=("n1", "n2", "n3", "n31", "n32", "n33", "star40", "k4", "path5", "free5",
                                                    "iso40", "two70")))
    cap = W.node_capacity(big)
    pe = _pe(len(big_names), cap, hid)
    g1, g2 = _batch(big, cap, hid), _batch(big, cap, hid)
    pe(g1)
    pe(g2)
    pe.check_status(strict=True)
    N, n = int(big["node_off"][-1]), int(small["node_off"][-1])
    first = g1.pos_undirected[:N].clone()
    assert g1.pos_undirected.data_ptr() != g2.pos_undirected.data_ptr()
    assert bool((first[:n, hid - 1] != 0).any()), "the large batch left nothing in the padding columns the small one must clear"
    # the small batch: same batch_size (the rest of the batch are empty items), same ring slot as g1
    no = np.r_[small["node_off"].numpy(), np.full(len(big_names) - len(names), n)]
    padded = dict(small, node_off=torch.from_numpy(no))
    g3 = _batch(padded, cap, hid)
    evals = torch.zeros(len(big_names), hid, device="cuda")
    raw = torch.zeros(cap, hid, device="cuda")
    pe(g3, evals=evals, raw=raw)
    pe.check_status(strict=True)
    assert g3.pos_undirected.data_ptr() == g1.pos_undirected.data_ptr()
    x = g3.pos_undirected[:n].cpu().numpy()
    fresh = _pe(len(big_names), cap, hid)
    g4 = _batch(padded, cap, hid)
    fresh(g4)
    fresh.check_status(strict=True)
    assert np.array_equal(x.view(np.uint32), g4.pos_undirected[:n].cpu().numpy().view(np.uint32))
    nos = small["node_off"].numpy()
    for b in range(len(names)):
        k = max(min(int(nos[b + 1] - nos[b]) - 2, hid), 0)
        assert not x[nos[b]:nos[b + 1], k:].any(), names[b]
    W.check_batch(names, small, hid, x, evals[:len(names)].cpu().numpy(), raw[:n].cpu().numpy())
    # rows the small batch does not own are untouched: still the large batch's
    assert torch.equal(g3.pos_undirected[n:N], first[n:N])
