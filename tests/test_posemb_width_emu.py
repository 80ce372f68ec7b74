"""The positional-embedding solver at widths below 32, into pre-filled output buffers, on disconnected graphs and isolated
nodes -- on the wave64 emulator (cases, checker and bars: tests/posemb_width_check.py).  Widths 2, 5, 16, 17, 30, 31 for every
class up to the block / slot classes; the 385..704 class and the Krylov class (the emulator's slowest items) at width 6."""
import ctypes

import pytest
import torch

from gcc_amd import _cabi
from gcc_amd.posemb import DevicePosEmb
from tests import posemb_width_check as W
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_encoder import CpuBatch


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _batch(view, cap, hid):
    return CpuBatch(dict(view, pos_undirected=torch.zeros(int(view["node_off"][-1]), hid)), node_cap=cap)


def _pe(B, cap, hid):
    return DevicePosEmb(B, cap, hid, device="cpu", lib=emu_lib(), ptr=_ptr, num_buffers=1)


def _run(named, hid, knob):
    names, view = W.batch(named)
    with W.Knobs(knob):
        x, evals, raw, status = W.run_filled(view, hid, _batch, _pe)
    cls = W.expected_status(names, view, knob, status)
    W.check_batch(names, view, hid, x, evals, raw)
    return dict(zip(names, cls))


def test_cases_cpu_only():
    """no kernel: the class every item reaches, the Gram-eligible set, the isolated-node condition (float64 only)"""
    W.check_cases()


@pytest.mark.parametrize("hid", W.EMU_WIDTHS)
def test_every_class_up_to_the_block_class(hid):
    """default knobs: the k edge, one-wave teams of 48 and 64, the four-wave 65..128 class, the block class, the degenerate
    spectra and the disconnected items"""
    cls = _run(W.width_items(hid), hid, "default")
    assert {"zeros", "w48", "w64", "pair", "block"} <= set(cls.values()), cls


@pytest.mark.parametrize("hid", W.EMU_WIDTHS)
@pytest.mark.parametrize("knob,only,reached", [
    ("wave0", ("wave40", "wave60", "iso40", "free5", "star40"), "small"),
    ("pair0", ("mid110", "two70"), "mid"),
    ("cheb0", ("sparse160", "iso155"), "slot")])
def test_the_classes_behind_the_knobs(knob, only, reached, hid):
    """GCC_POSEMB_WAVE=0: the 256-thread small class; GCC_POSEMB_PAIR=0: the 1,024-thread 65..128 class; GCC_POSEMB_CHEB=0: the
    129..384 slot class -- each with the k-edge items beside its own"""
    named = W.width_items(hid, only=tuple(W.kedge_items(hid)) + only)
    cls = _run(named, hid, knob)
    assert all(cls[nm] == reached for nm in only), cls


def test_big_and_krylov_classes_at_width_6():
    """GCC_POSEMB_CHEB=0: skewed_dense_graph(400) in the 385..704 class; skewed_dense_graph(760), alone and with three isolated
    nodes, and the eight-community graph with three isolated nodes in the Krylov class (8-column output chunks: 6 is less
    than one)"""
    hid = W.EMU_BIG_WIDTH
    cls = _run(W.width_items(hid, heavy=True, only=W.HEAVY), hid, "cheb0")
    assert cls == dict(big400="big", kry760="krylov", iso763="krylov", comm763="krylov")


@pytest.mark.parametrize("hidden", [1, 33])
def test_widths_outside_2_to_32_are_refused_by_name(hidden):
    lib = emu_lib()
    assert lib.gcc_posemb_multi_workspace_bytes(1, 2, 64, hidden) == -1
    assert lib.gcc_last_error().decode() == "gcc_posemb_multi_workspace_bytes: bad argument"
    names, view = W.batch(W.width_items(2, only=("n3", "n4")))
    g = _batch(view, 64, 32)
    out = torch.full((64, 33), W.SENTINEL)
    evals, raw = torch.full((2, 33), W.SENTINEL), torch.full((64, 33), W.SENTINEL)
    ws = torch.full((lib.gcc_posemb_multi_workspace_bytes(1, 2, 64, 2),), 0xA5, dtype=torch.uint8)
    status = torch.zeros(16, dtype=torch.int32)
    c = _cabi.batch_out(g, _ptr, 64, csr_only=True)
    v = (_cabi.GccPosembView * 1)(_cabi.GccPosembView(g=ctypes.addressof(c), pos=_ptr(out), evals=_ptr(evals), raw=_ptr(raw)))
    rc = lib.gcc_posemb_multi(v, 1, 2, 64, hidden, 0, _ptr(ws), ws.numel(), _ptr(status), None, None)
    assert rc != 0 and lib.gcc_last_error().decode() == "gcc_posemb_multi: bad argument"
    for t in (out, evals, raw):
        assert bool((t == W.SENTINEL).all())
    assert bool((ws == 0xA5).all()) and not status.any()
