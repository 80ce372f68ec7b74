"""gcc_graph_build / gcc_graph_check (gcc_amd/csrc/graph_build.hip) against the NumPy restatement of the converter's rule
(gcc_amd.graph_build.build_csr_numpy), shared by the emulator tier (tests/test_graph_build_emu.py) and the GPU tier
(tests/test_graph_build_gpu.py): the same cases and checks; only the library, the pointer function and the device differ.

Every comparison is exact integer equality.  The shapes come from the class boundaries the library exports (_cabi.GRAPH_BUILD_*):
a row of 64 slots is a wave's, one of GRAPH_BUILD_LDS_ROW a workgroup's, a longer one is sorted in chunks and merged; the scans
work on tiles of GRAPH_BUILD_SCAN_TILE.  The outputs are allocated with guard words on both sides and pre-filled, so a write outside
the documented extent, or a reliance on the unused tails, shows."""
import ctypes

import numpy as np
import pytest
import torch

from gcc_amd import _cabi
from gcc_amd import graph_build as GB
from gcc_amd.graph_build import GraphBuildEngine, build_csr_numpy
from gcc_amd.graphgen import check_contract, check_multigraph_contract

T, L, W = _cabi.GRAPH_BUILD_SCAN_TILE, _cabi.GRAPH_BUILD_LDS_ROW, _cabi.GRAPH_BUILD_WAVE_ROW
GUARD, FILL, G = 0x6B6B6B6B, 0x5A5A5A5A, 8
HUB_SIZES = (W - 1, W, W + 1, L - 1, L, L + 1, 2 * L + 3)


def star(h, hub=0):
    """the hub and every other id of 0..h, the hub second in every other line"""
    leaves = np.delete(np.arange(h + 1), hub)
    lines = np.stack([np.full(h, hub), leaves], axis=1)
    lines[1::2] = lines[1::2, ::-1]
    return lines


def straddling(h):
    """a star whose repeats stand a whole chunk of the large class after their first copy: the two copies of a neighbour are
    sorted in different chunks (the emulator keeps the lines' order in a row) and meet only in a merge"""
    base = star(h)
    parts, at = [], 0
    while at < len(base):
        parts.append(base[at:at + L - 4])
        if at:
            parts.append(base[at - 3:at + 1][:, ::-1])          # (repeats of the entries around the last chunk's end)
        at += L - 4
    parts.append(base[:2])
    return np.concatenate(parts)


def powerlaw_lines(n, m, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    w = (np.arange(n) + 1.0) ** -0.8
    return rng.choice(n, size=(m, 2), p=w / w.sum())


def random_lines(n, m, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, n, size=(m, 2))


def make_cases():
    c = {}
    c["m0"] = (5, np.zeros((0, 2), dtype=np.int64))
    c["n1_m0"] = (1, np.zeros((0, 2), dtype=np.int64))
    c["n1_loop"] = (1, np.array([[0, 0]]))
    c["one_line"] = (3, np.array([[2, 0]]))
    c["only_loops"] = (4, np.array([[1, 1], [2, 2], [1, 1]]))
    c["one_edge_ten_times"] = (6, np.array([[1, 4], [4, 1]] * 5))
    c["unused_nodes"] = (10, np.array([[2, 5], [7, 5], [5, 2], [7, 2]]))
    c["loop_only_node"] = (5, np.array([[0, 1], [3, 3], [1, 2], [3, 3]]))
    for n in (T - 1, T, T + 1):
        c[f"n{n}"] = (n, random_lines(n, n // 2, n))            # (about a third of the nodes unused: node_map crosses the tile)
    for m in (T - 1, T, T + 1):
        c[f"m{m}"] = (300, random_lines(300, m, m))
    for h in HUB_SIZES:
        c[f"star{h}"] = (h + 1, star(h))
        c[f"star{h}x3"] = (h + 3, np.random.Generator(np.random.PCG64(h)).permutation(np.repeat(star(h, hub=2), 3, axis=0)))
        c[f"star{h}straddle"] = (h + 1, straddling(h))
    c["lds_class_before_wave_class_after"] = (60, np.repeat(star(40), 2, axis=0))
    c["large_class_before_lds_class_after"] = (L // 2 + 20, np.tile(star(L // 2 + 10), (2, 1)))
    c["powerlaw"] = (2000, powerlaw_lines(2000, 12000, 7))
    return c


CASES = make_cases()
NAMES = list(CASES)
_REFERENCE = {}


def reference(name):
    """build_csr_numpy of a case, computed once and handed out read-only"""
    if name not in _REFERENCE:
        n, lines = CASES[name]
        ref = build_csr_numpy(lines, n)
        for v in ref.values():
            v.setflags(write=False)
        _REFERENCE[name] = ref
    return _REFERENCE[name]


class Gb:
    """the library under test, its pointer function and its device (the emulator works on CPU tensors)"""

    def __init__(self, lib, ptr, device):
        self.lib, self.ptr, self.device = lib, ptr, torch.device(device)
        self.engine = GraphBuildEngine(lib, ptr, device)

    def guarded(self, words, dtype=torch.int32):
        t = torch.full((words + 2 * G,), FILL, dtype=dtype, device=self.device)
        t[:G] = GUARD
        t[G + words:] = GUARD
        return t

    def build(self, lines, n):
        """the bare call into guarded, pre-filled buffers -> the outputs as numpy, sliced by counts"""
        lines = np.asarray(lines).reshape(-1, 2)
        m = len(lines)
        pairs = torch.from_numpy(np.ascontiguousarray(lines.astype(np.int32))).to(self.device)
        rp, ci, nm = self.guarded(n + 1), self.guarded(2 * m), self.guarded(n)
        counts = torch.full((6,), -1, dtype=torch.int64, device=self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.engine.build_into(pairs, n, rp[G:G + n + 1], ci[G:G + 2 * m], nm[G:G + n], counts, status)
        rp, ci, nm, counts = rp.cpu().numpy(), ci.cpu().numpy(), nm.cpu().numpy(), counts.cpu().numpy()
        for buf, words in ((rp, n + 1), (ci, 2 * m), (nm, n)):
            assert (buf[:G] == GUARD).all() and (buf[G + words:] == GUARD).all(), "a guard word was written"
        kept, entries = int(counts[0]), int(counts[1])
        assert 0 <= kept <= n and 0 <= entries <= 2 * m
        assert (rp[G + kept + 1:G + n + 1] == FILL).all() and (ci[G + entries:G + 2 * m] == FILL).all()   # (the tails are left alone)
        return dict(row_ptr=rp[G:G + kept + 1], col_idx=ci[G:G + entries], node_map=nm[G:G + n], counts=counts,
                    status=status.cpu().numpy())

    def check(self, row_ptr, col_idx, multigraph=False):
        res = self.engine.check(np.asarray(row_ptr, dtype=np.int32), np.asarray(col_idx, dtype=np.int32), multigraph)
        return int(res["status"].cpu()[0]), [int(x) for x in res["maxima"].cpu()]


def same(got, ref, what=""):
    for key in ("counts", "status", "row_ptr", "col_idx", "node_map"):
        assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), (what, key)


def check_parity(gb, name):
    n, lines = CASES[name]
    ref = reference(name)
    got = gb.build(lines, n)
    same(got, ref, name)
    assert int(got["status"][0]) == 0
    kept, entries, loops, dups, dropped, longest = (int(x) for x in got["counts"])
    # the counts against their definitions, on the input itself
    u, v = np.asarray(lines)[:, 0], np.asarray(lines)[:, 1]
    assert loops == int((u == v).sum()) and dups == 2 * int((u != v).sum()) - entries and dropped == n - kept
    used = np.zeros(n, dtype=bool)
    used[u[u != v]] = True
    used[v[u != v]] = True
    assert kept == int(used.sum())
    nm = got["node_map"]
    assert (nm[~used] == -1).all() and np.array_equal(nm[used], np.arange(kept))        # monotone on the survivors
    if kept:
        rp, ci = got["row_ptr"], got["col_idx"]
        check_contract(rp, ci)
        assert longest == int(np.diff(rp).max())
        status, maxima = gb.check(rp, ci)
        assert status == 0 and maxima == [longest, 1]
    else:
        assert entries == 0 and longest == 0 and np.array_equal(got["row_ptr"], [0])


def check_order_independence(gb, name, calls=1):
    """the same lines in another order (and each line's ends swapped at random) give the same bits; ``calls`` > 1: so does the same
    call again (on the device the rows fill in whatever order the atomics arrive)"""
    n, lines = CASES[name]
    ref = reference(name)
    rng = np.random.Generator(np.random.PCG64(11))
    for _ in range(calls):
        same(gb.build(lines, n), ref, name)
    shuffled = rng.permutation(np.asarray(lines), axis=0)
    flip = rng.random(len(shuffled)) < 0.5
    shuffled[flip] = shuffled[flip][:, ::-1]
    same(gb.build(shuffled, n), ref, name + " shuffled")


def check_bad_ids(gb):
    """ids of -1 and n set the bit; the other lines build their graph"""
    n, lines = CASES["m%d" % T]
    bad = np.array([[-1, 3], [4, n], [n, n], [-1, -1], [2 ** 31 - 1, 0], [0, -2 ** 31]])
    mixed = np.concatenate([lines[:100], bad[:3], lines[100:], bad[3:]])
    ref = build_csr_numpy(mixed, n)
    assert int(ref["status"][0]) == _cabi.STATUS_GRAPH_BUILD_BAD_ID
    got = gb.build(mixed, n)
    same(got, ref)
    clean = reference("m%d" % T)
    for key in ("row_ptr", "col_idx", "node_map", "counts"):
        assert np.array_equal(got[key], clean[key]), key
    with pytest.raises(RuntimeError, match="outside \\[0, n\\)"):
        gb.engine.check_status(dict(status=torch.from_numpy(got["status"])))


def check_refusals(gb):
    dev = gb.device
    pairs = torch.zeros((4, 2), dtype=torch.int32, device=dev)
    bufs = dict(row_ptr=torch.zeros(6, dtype=torch.int32, device=dev), col_idx=torch.zeros(8, dtype=torch.int32, device=dev),
                node_map=None, counts=torch.full((6,), -1, dtype=torch.int64, device=dev),
                status=torch.zeros(1, dtype=torch.int32, device=dev))
    for member in ("row_ptr", "col_idx", "counts"):
        with pytest.raises(RuntimeError, match=f"gcc_graph_build.*{member} is NULL"):
            gb.engine.build_into(pairs, 5, **{**bufs, member: None})
    with pytest.raises(RuntimeError, match="gcc_graph_build.*pairs is NULL"):
        a = _cabi.GccGraphBuildArgs(n=5, m=4, row_ptr=gb.ptr(bufs["row_ptr"]), col_idx=gb.ptr(bufs["col_idx"]), counts=gb.ptr(bufs["counts"]))
        gb.engine.invoke("gcc_graph_build", a, gb.engine.workspace(1 << 16, dev), bufs["status"])
    with pytest.raises(RuntimeError, match="workspace_bytes 64 is less than gcc_graph_build_workspace_bytes"):
        gb.engine.build_into(pairs, 5, **bufs, workspace_bytes=64)
    assert gb.lib.gcc_graph_build_workspace_bytes(5, 2 ** 30) < 0 and b"2 m must stay below 2^31" in gb.lib.gcc_last_error()
    assert gb.lib.gcc_graph_build_workspace_bytes(2 ** 31, 4) < 0 and b"node ids are int32" in gb.lib.gcc_last_error()
    assert gb.lib.gcc_graph_build_workspace_bytes(0, 4) < 0
    assert gb.lib.gcc_graph_build_workspace_bytes(2 ** 31 - 1, 2 ** 30 - 1) > 0
    with pytest.raises(RuntimeError, match="2 m must stay below 2\\^31"):
        a = _cabi.GccGraphBuildArgs(pairs=gb.ptr(pairs), n=5, m=2 ** 30, row_ptr=gb.ptr(bufs["row_ptr"]), col_idx=gb.ptr(bufs["col_idx"]),
                                    counts=gb.ptr(bufs["counts"]))
        gb.engine.invoke("gcc_graph_build", a, gb.engine.workspace(1 << 16, dev), bufs["status"])
    c = _cabi.GccGraphCheckArgs(n=5, nnz=8, col_idx=gb.ptr(bufs["col_idx"]), maxima=gb.ptr(bufs["row_ptr"]))
    with pytest.raises(RuntimeError, match="gcc_graph_check.*row_ptr is NULL"):
        gb.engine.invoke("gcc_graph_check", c, gb.engine.workspace(256, dev), bufs["status"])
    c.row_ptr, c.maxima = gb.ptr(bufs["row_ptr"]), None
    with pytest.raises(RuntimeError, match="gcc_graph_check.*maxima is NULL"):
        gb.engine.invoke("gcc_graph_check", c, gb.engine.workspace(256, dev), bufs["status"])
    assert int(bufs["status"].cpu()[0]) == 0 and (bufs["counts"].cpu().numpy() == -1).all()       # (nothing was launched)
    assert ctypes.sizeof(_cabi.GccGraphBuildArgs) % 8 == 0 and ctypes.sizeof(_cabi.GccGraphCheckArgs) % 8 == 0


def check_cpu_tensor_refused(lib):
    eng = GraphBuildEngine(lib, _cabi.dev_ptr, "cpu")
    with pytest.raises(RuntimeError, match="device \\(HIP\\) tensors only"):
        eng.build(np.array([[0, 1]]), 2)
    with pytest.raises(RuntimeError, match="device \\(HIP\\) tensors only"):
        eng.check(np.array([0, 1, 2]), np.array([1, 0]))


def violations():
    """an otherwise valid CSR with ONE violation each -> {name: (row_ptr, col_idx, the bit)}"""
    ref = reference("powerlaw")
    rp, ci = ref["row_ptr"].astype(np.int64), ref["col_idx"].copy()
    n = len(rp) - 1
    row = int(np.argmax(np.diff(rp)))                               # the longest row, and its first two entries
    at = int(rp[row])
    out = {}
    bad = ci.copy()
    bad[[at, at + 1]] = ci[[at + 1, at]]
    out["swapped_pair"] = (rp, bad, _cabi.STATUS_GRAPH_CHECK_UNSORTED)
    grown = rp.copy()
    grown[row + 1:] += 1
    out["duplicated_entry"] = (grown, np.insert(ci, at, ci[at]), _cabi.STATUS_GRAPH_CHECK_DUPLICATE)
    pos = int(np.searchsorted(ci[rp[row]:rp[row + 1]], row))
    out["self_loop"] = (grown, np.insert(ci, at + pos, row), _cabi.STATUS_GRAPH_CHECK_SELF_LOOP)
    shrunk = rp.copy()
    shrunk[row + 1:] -= 1
    out["one_direction_removed"] = (shrunk, np.delete(ci, at), _cabi.STATUS_GRAPH_CHECK_ASYMMETRIC)
    out["empty_row"] = (np.append(rp, rp[-1]), ci, _cabi.STATUS_GRAPH_CHECK_ZERO_DEGREE)
    last = rp.copy()
    last[-1] += 1
    out["column_n"] = (last, np.append(ci, n), _cabi.STATUS_GRAPH_CHECK_RANGE)
    out["row_ptr_stops_short"] = (rp, np.append(ci, 0), _cabi.STATUS_GRAPH_CHECK_SPAN)
    return out


def check_violation(gb, name):
    rp, ci, bit = violations()[name]
    with pytest.raises(ValueError) as err:
        check_contract(rp.astype(np.int32), ci.astype(np.int32))
    status, _ = gb.check(rp, ci)
    assert status == bit, (name, status)
    assert GB.contract_error(status) == str(err.value)              # the host check's own message
    with pytest.raises(ValueError) as dev_err:
        gb.engine.validate(rp.astype(np.int32), ci.astype(np.int32))
    assert str(dev_err.value) == str(err.value)


def check_multigraph_mode(gb):
    from tests import multigraph_cases as M

    ref = reference("powerlaw")
    rp, ci = ref["row_ptr"].astype(np.int64), ref["col_idx"]
    # every entry three times: equal copy counts in both directions
    rp3, ci3 = 3 * rp, np.repeat(ci, 3)
    check_multigraph_contract(rp3.astype(np.int32), ci3)
    assert gb.check(rp3, ci3, multigraph=True) == (0, [3 * int(ref["counts"][5]), 3])
    assert gb.check(rp3, ci3)[0] == _cabi.STATUS_GRAPH_CHECK_DUPLICATE
    # one more copy in one direction only
    row = int(np.argmax(np.diff(rp)))
    grown = rp3.copy()
    grown[row + 1:] += 1
    lop = np.insert(ci3, int(rp3[row]), ci3[int(rp3[row])])
    with pytest.raises(ValueError, match="equal copy counts"):
        check_multigraph_contract(grown.astype(np.int32), lop)
    status, _ = gb.check(grown, lop, multigraph=True)
    assert status == _cabi.STATUS_GRAPH_CHECK_ASYMMETRIC
    assert GB.contract_error(status, multigraph=True).startswith("graph is not symmetric with equal copy counts")
    # the weighted parent the multigraph tests walk: copy counts 1..5, equal in both directions
    mrp, mci = M.weighted_parent(ref["row_ptr"], ref["col_idx"], np.random.RandomState(5))
    check_multigraph_contract(mrp, mci)
    assert gb.check(mrp, mci, multigraph=True) == (0, [int(np.diff(mrp).max()), 5])
