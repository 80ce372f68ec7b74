"""gcc_text_ints_sep, gcc_tu_corpus, TUIngestEngine and DeviceGraphCorpus.from_device (gcc_amd/csrc/text_ingest.hip,
gcc_amd/csrc/tu_corpus.hip, gcc_amd/tu_ingest.py, gcc_amd/datasets.py) against the host route, shared by the emulator tier
(tests/test_tu_ingest_emu.py) and the GPU tier (tests/test_tu_ingest_gpu.py): the same cases and checks; only the library, the
pointer function, the device and the number of calls differ (the GPU tier makes every call twice and compares the bits).

The two yardsticks are existing code: ``ingest.read_tudataset`` on the same files, and ``DeviceGraphCorpus(graphs, ...)`` on its
output.  For the tokenizer, ``model`` restates the token rule of include/gcc_amd.h with a regular expression and is itself held
against ``np.loadtxt(delimiter=",")`` on every text NumPy can read.  Equality is exact everywhere.

Sizes come from the exported constants: T = TEXT_TILE_BYTES, a lane's span of 16, a wave's of 1,024; the row classes
GRAPH_BUILD_WAVE_ROW / GRAPH_BUILD_LDS_ROW and the scan tile GRAPH_BUILD_SCAN_TILE."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

from gcc_amd import _cabi, ingest
from gcc_amd.datasets import DeviceGraphCorpus
from gcc_amd.text_ingest import TextIngestEngine
from gcc_amd.tu_ingest import TUIngestEngine
from tests.text_ingest_check import FILL, G, GUARD, make_text

T = _cabi.TEXT_TILE_BYTES
LANE, WAVE = 16, 1024
WAVE_ROW, LDS_ROW, SCAN_TILE = _cabi.GRAPH_BUILD_WAVE_ROW, _cabi.GRAPH_BUILD_LDS_ROW, _cabi.GRAPH_BUILD_SCAN_TILE
NOT_INT, RANGE, SHORT, SHAPE = (_cabi.STATUS_TEXT_NOT_INTEGER, _cabi.STATUS_TEXT_INT32_RANGE, _cabi.STATUS_TEXT_SHORT,
                                _cabi.STATUS_TEXT_LINE_SHAPE)
SIX = b"\t\n\x0b\x0c\r "
INTEGER = re.compile(rb"[+-]?[0-9]+")
NAME = "UNIT"
TABLES = ("node_first", "edge_first", "row_ptr", "col_idx", "seed_local", "labels")


# ---------------------------------------------------------------------------------------------------------------- the tokenizer
def model(data, first, max_tokens, fields, keep, extra, line_records):
    """the token rule restated -> (flat expected words with FILL where nothing is stored, summary [4], status)"""
    data = bytes(data)
    token = re.compile(b"[^" + re.escape(SIX + (bytes([extra]) if extra else b"")) + b"]+")
    words = np.full(max_tokens // fields * keep, FILL, dtype=np.int64)
    bad, out_of_range, shape, r, before = [], [], [], -1, first
    for r, mt in enumerate(token.finditer(data, first)):
        if r < max_tokens:
            ok = INTEGER.fullmatch(mt.group()) is not None
            if not ok:
                bad.append(mt.start())
            if line_records and (r == 0 or b"\n" in data[before:mt.start()]) != (r % fields == 0):
                shape.append(mt.start())
            if r % fields < keep:
                v = int(mt.group()) if ok else 0
                if not -2 ** 31 <= v < 2 ** 31:
                    out_of_range.append(mt.start())
                    v = 0
                words[r // fields * keep + r % fields] = v
        before = mt.end()
    total = r + 1
    status = (NOT_INT if bad else 0) | (RANGE if out_of_range else 0) | (SHORT if total < max_tokens else 0) | (SHAPE if shape else 0)
    return words, [total, min(bad, default=-1), min(out_of_range, default=-1), min(shape, default=-1) if line_records else 0], status


class Tu:
    """the library under test, its pointer function and its device (the emulator works on CPU tensors); ``calls``: how often every
    call is made (their bits must agree)"""

    def __init__(self, lib, ptr, device, calls=1):
        self.lib, self.ptr, self.device, self.calls = lib, ptr, torch.device(device), calls
        self.text = TextIngestEngine(lib, ptr, device)
        self.engine = TUIngestEngine(lib, ptr, device, text_engine=self.text)

    def upload(self, data):
        text, nbytes = self.text.upload(bytes(data))
        text[nbytes:] = ord("7")                                    # what lies at and above nbytes must not matter
        return text, nbytes

    def _guarded(self, call, words):
        seen = []
        for _ in range(self.calls):
            out = torch.full((words + 2 * G,), FILL, dtype=torch.int32, device=self.device)
            out[:G] = GUARD
            out[G + words:] = GUARD
            summary = torch.full((4,), -7, dtype=torch.int64, device=self.device)
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            call(out[G:G + words], summary, status)
            o = out.cpu().numpy()
            assert (o[:G] == GUARD).all() and (o[G + words:] == GUARD).all(), "a guard word was written"
            seen.append((o[G:G + words].astype(np.int64), [int(x) for x in summary.cpu()], int(status.cpu()[0])))
        for other in seen[1:]:
            assert np.array_equal(other[0], seen[0][0]) and other[1:] == seen[0][1:], "two calls differ"
        return seen[0]

    def ints_sep(self, data, first, max_tokens, fields, keep, extra=0, line_records=0):
        text, nbytes = self.upload(data)
        return self._guarded(lambda o, s, st: self.text.ints_sep_into(text, nbytes, first, max_tokens, fields, keep, o, s, st, extra,
                                                                      line_records), max_tokens // fields * keep)

    def ints(self, data, first, max_tokens, fields, keep):
        text, nbytes = self.upload(data)
        return self._guarded(lambda o, s, st: self.text.ints_into(text, nbytes, first, max_tokens, fields, keep, o, s, st),
                             max_tokens // fields * keep)

    def held(self, data, first, max_tokens, fields, keep, extra, line_records):
        got = self.ints_sep(data, first, max_tokens, fields, keep, extra, line_records)
        want = model(data, first, max_tokens, fields, keep, extra, line_records)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2], (got[1:], want[1:])
        return got


def check_knobs_off(tu):
    """with both knobs off the new entry gives the old entry's words, on generated texts of every separator"""
    for nbytes, seed, first, fields, keep in ((700, 1, 0, 3, 2), (T + 37, 2, 5, 1, 1), (3 * T, 3, T - 1, 4, 4), (2 * T + 1, 4, 0, 2, 1)):
        data = make_text(nbytes, seed)
        total = len(bytes(data[first:]).split())
        for max_tokens in (total // fields * fields, (total // fields + 2) * fields, fields):
            old = tu.ints(data, first, max_tokens, fields, keep)
            new = tu.ints_sep(data, first, max_tokens, fields, keep, 0, 0)
            assert np.array_equal(old[0], new[0]) and old[1] == new[1] and old[2] == new[2] and old[1][3] == 0
            assert new[2] & SHAPE == 0


def loadtxt_pairs(data):
    return np.loadtxt(io.BytesIO(bytes(data)), delimiter=",", dtype=np.int64, ndmin=2)


def check_comma_forms(tu):
    """``u, v``, ``u,v`` and ``u ,v``; CRLF line ends, no final newline, blank lines: the host reader's values, a clean word"""
    for text in (b"1, 2\n3, 4\n", b"1,2\n3,4\n", b"1 ,2\n3 , 4\n", b"1, 2\r\n3,4\r\n", b"1, 2\n3, 4", b"\n\n1, 2\n\n\n3, 4\n\n", b"-5,+6\n007, 8",
                 b"12345, 678\n" * 40):
        want = loadtxt_pairs(text)
        words, summary, status = tu.held(text, 0, 2 * len(want), 2, 2, 44, 1)
        assert status == 0 and summary == [2 * len(want), -1, -1, -1]
        assert np.array_equal(words.reshape(-1, 2), want)
    # without the knob a comma is part of its token; two commas are one separator run
    assert tu.held(b"1,2\n", 0, 2, 2, 2, 0, 0)[2] == NOT_INT | SHORT
    assert tu.held(b"1,,2\n3 4\n", 0, 4, 2, 2, 44, 1)[2] == 0
    # any other byte may be the seventh separator
    assert tu.held(b"1;2\n3;4\n", 0, 4, 2, 2, ord(";"), 1)[2] == 0
    assert tu.held(b"1\x002\n", 0, 2, 2, 2, 0, 0)[2] == NOT_INT | SHORT and tu.held(b"1\xff2\n", 0, 2, 2, 2, 255, 1)[2] == 0


SEAMS = {f"{name}_{side}": (at, side) for name, at in (("lane", LANE), ("wave", WAVE), ("tile", T), ("tile2", 2 * T))
         for side in ("before", "after")}


def check_comma_seam(tu, name):
    """a comma as the last byte before a seam and as the first byte after it, its two tokens on the two sides"""
    at, side = SEAMS[name]
    comma = at - 1 if side == "before" else at
    head = b"1,2\n" * ((comma - 2) // 4)
    head += b" " * (comma - 2 - len(head))
    text = head + b"34,56\n" + b"7, 8\n" * 30
    assert text[comma] == 44 and text[comma - 2:comma] == b"34"
    want = loadtxt_pairs(text)
    words, summary, status = tu.held(text, 0, 2 * len(want), 2, 2, 44, 1)
    assert status == 0 and np.array_equal(words.reshape(-1, 2), want)
    # the comma between two spaces, and the token right behind the seam's comma
    text2 = head + b"34 , 56\n" if side == "before" else head[:-1] + b"34 ,56\n"
    tu.held(text2 + b"9,9\n", 0, len((text2 + b"9,9\n").replace(b",", b" ").split()), 2, 2, 44, 1)


def check_newline_in_the_previous_tile(tu):
    """a separator run whose newline lies in the tile before the token: the token is still the first on its line"""
    for gap in (1, 3, LANE + 2):
        head = b"1,2\n" * ((T - gap) // 4 - 1)
        head += b"1," + b"2" * (T - gap - len(head) - 3) + b"\n"      # the newline at T - gap - 1
        text = head + b" " * gap + b"3,4\n5,6\n"
        assert text[T - gap - 1] == 10 and text[T] == ord("3")
        words, summary, status = tu.held(text, 0, 2 * text.count(b"\n"), 2, 2, 44, 1)
        assert status & SHAPE == 0 and summary[3] == -1
        # the same run without its newline: one line of four tokens
        flat = head[:-1] + b" " + b" " * gap + b"3,4\n5,6\n"
        _, summary, status = tu.held(flat, 0, 2 * flat.count(b"\n") + 2, 2, 2, 44, 1)
        assert status & SHAPE and summary[3] == T


def check_line_records(tu):
    good = b"1,2\n" * 5
    three, one = b"1,2,3\n", b"9\n"
    for text, at in ((good + three + good, len(good) + 4), (good + one + good, len(good) + len(one)),
                     (good + one + good + three, len(good) + len(one)), (good + three + one + good, len(good) + 4)):
        total = len(text.replace(b",", b" ").split())
        _, summary, status = tu.held(text, 0, total // 2 * 2, 2, 2, 44, 1)
        assert status & SHAPE and summary[3] == at, (text, summary)
        # nothing behind max_tokens is looked at
        _, summary, status = tu.held(text, 0, 10, 2, 2, 44, 1)
        assert status == 0 and summary[3] == -1
        # without line_records the same text is just tokens
        _, summary, status = tu.held(text, 0, total // 2 * 2, 2, 2, 44, 0)
        assert status == 0 and summary[3] == 0
    # one integer per line; first_byte inside the text: the first token at or after it opens the first record
    assert tu.held(b"3\n3\n\n7\n", 0, 3, 1, 1, 0, 1)[2] == 0
    assert tu.held(b"3\n3 7\n", 0, 3, 1, 1, 0, 1)[1][3] == 4
    assert tu.held(b"5 1,2\n3,4\n", 2, 4, 2, 2, 44, 1)[2] == 0


def check_count_only(tu):
    """out == NULL, max_tokens == 0: the tokens under the seven separators"""
    for text, extra, want in ((b"1,2\n3, 4\n5 ,6", 44, 6), (b"1,2\n3, 4\n", 0, 3), (b",,,\n", 44, 0), (make_text(T + 5, 9).tobytes(), 0, None)):
        t, nbytes = tu.upload(text)
        for _ in range(tu.calls):
            summary = torch.full((4,), -7, dtype=torch.int64, device=tu.device)
            status = torch.zeros(1, dtype=torch.int32, device=tu.device)
            tu.text.ints_sep_into(t, nbytes, 0, 0, 2, 2, None, summary, status, extra, 1)
            assert [int(x) for x in summary.cpu()] == [len(text.split()) if want is None else want, -1, -1, -1] and int(status.cpu()[0]) == 0


def check_extra_sep_refused(tu):
    t, nbytes = tu.upload(b"1,2\n")
    summary = torch.full((4,), -7, dtype=torch.int64, device=tu.device)
    status = torch.zeros(1, dtype=torch.int32, device=tu.device)
    out = torch.full((2,), FILL, dtype=torch.int32, device=tu.device)
    for extra in (ord("0"), ord("5"), ord("9"), ord("+"), ord("-"), 9, 10, 11, 12, 13, 32, 256, -1):
        with pytest.raises(RuntimeError, match=f"gcc_text_ints_sep.*extra_sep {extra}:"):
            tu.text.ints_sep_into(t, nbytes, 0, 2, 2, 2, out, summary, status, extra, 0)
    with pytest.raises(RuntimeError, match="gcc_text_ints_sep.*line_records 2 is neither 0 nor 1"):
        tu.text.ints_sep_into(t, nbytes, 0, 2, 2, 2, out, summary, status, 44, 2)
    with pytest.raises(RuntimeError, match="gcc_text_ints_sep.*out is NULL"):
        tu.text.ints_sep_into(t, nbytes, 0, 2, 2, 2, None, summary, status, 44, 1)
    with pytest.raises(RuntimeError, match="gcc_text_ints_sep.*workspace_bytes 8 is less than gcc_text_ints_workspace_bytes"):
        tu.text.ints_sep_into(t, nbytes, 0, 2, 2, 2, out, summary, status, 44, 1, workspace_bytes=8)
    assert int(status.cpu()[0]) == 0 and (out.cpu().numpy() == FILL).all() and (summary.cpu().numpy() == -7).all()


# ---------------------------------------------------------------------------------------------------------------- the build
def dataset(graphs, labels, gids=None):
    """``graphs``: [(nodes, [(a, b) undirected, local ids])] -> (pairs int64 [m, 2] 1-based, both directions; indicator; labels)"""
    pairs, indicator, first = [], [], 0
    gids = list(range(1, len(graphs) + 1)) if gids is None else gids
    for (n, edges), gid in zip(graphs, gids):
        for a, b in edges:
            pairs += [(first + a + 1, first + b + 1), (first + b + 1, first + a + 1)]
        indicator += [gid] * n
        first += n
    return np.array(pairs, dtype=np.int64).reshape(-1, 2), np.array(indicator, dtype=np.int64), np.array(labels, dtype=np.int64)


def star(leaves, hub_last=False):
    hub = leaves if hub_last else 0
    return leaves + 1, [(hub, i + (0 if hub_last else 1)) for i in range(leaves)]


def path(n):
    return n, [(i, i + 1) for i in range(n - 1)]


TRIANGLE = (3, [(0, 1), (1, 2), (0, 2)])


def two_node_graphs(count):
    return [(2, [(0, 1)])] * count


def _cases():
    c = {}
    c["one_graph_of_one_node"] = dataset([(1, [])], [5])
    c["isolated_first_last_and_last_in_file"] = dataset([(4, [(1, 2), (2, 3)]), (3, [(0, 1)]), TRIANGLE, (3, [(0, 1)])], [0, 1, 0, 1])
    c["edge_free_graph_in_the_middle_and_at_the_end"] = dataset([TRIANGLE, (2, []), TRIANGLE, (3, [])], [1, 1, 2, 2])
    c["indicator_3_3_7_7_7_20"] = dataset([(2, [(0, 1)]), path(3), (1, [])], [0, 1, 1], gids=[3, 7, 20])
    c["labels_minus_one_and_one"] = dataset([TRIANGLE, path(2), path(4)], [1, -1, 1])
    c["labels_single_class"] = dataset([TRIANGLE, path(2), path(4)], [7, 7, 7])
    c["labels_sparse_unsorted"] = dataset([TRIANGLE, path(2), path(4), path(3), (1, [])], [100, -7, 100, 3000000, -2 ** 31])
    c["seed_degree_tie_and_maximum_on_the_last_node"] = dataset([path(4), star(5, hub_last=True), (4, [(0, 1), (2, 3)]), star(3)], [0, 1, 0, 1])
    rows = (WAVE_ROW - 1, WAVE_ROW, WAVE_ROW + 1, LDS_ROW - 1, LDS_ROW, LDS_ROW + 1)
    c["star_rows_at_the_class_edges"] = dataset([star(k, hub_last=k % 2 == 1) for k in rows], [k % 3 for k in rows])
    for n in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
        c[f"nodes_{n}"] = dataset(two_node_graphs(n // 2) + [(1, [])] * (n % 2), [i % 2 for i in range(n // 2 + n % 2)])
        c[f"graphs_{n}"] = dataset(two_node_graphs(n), [(i * 7) % 5 - 2 for i in range(n)])
    many = LDS_ROW + 1                                              # the labels as one row of the third sort class
    c[f"labels_{many}"] = dataset(two_node_graphs(many), [(i * 7919) % 2053 - 1000 for i in range(many)])
    c["no_edge_at_all"] = dataset([(2, []), (1, []), (3, [])], [2, 0, 2])
    return c


CASES = _cases()


def write_files(folder, pairs, indicator, labels, seed=None, sep=", "):
    """the three files; the lines of A.txt in the order of a seeded permutation"""
    os.makedirs(folder, exist_ok=True)
    if seed is not None:
        pairs = pairs[np.random.Generator(np.random.PCG64(seed)).permutation(len(pairs))]
    base = os.path.join(str(folder), NAME + "_")
    with open(base + "A.txt", "w") as f:
        f.write("".join(f"{u}{sep}{v}\n" for u, v in pairs.tolist()))
    with open(base + "graph_indicator.txt", "w") as f:
        f.write("".join(f"{x}\n" for x in indicator.tolist()))
    with open(base + "graph_labels.txt", "w") as f:
        f.write("".join(f"{x}\n" for x in labels.tolist()))
    return str(folder)


def host_corpus(tu, folder, batch_size=4, **kw):
    """the two yardsticks: the host reader, then the host constructor"""
    if os.path.getsize(os.path.join(folder, NAME + "_A.txt")) == 0:
        # np.loadtxt gives an empty file the shape (0, 1) and the host reader stops at its second column: the edge-free dataset by
        # the reader's own rule for the two other files
        sizes = np.unique(np.loadtxt(os.path.join(folder, NAME + "_graph_indicator.txt"), dtype=np.int64, ndmin=1), return_counts=True)[1]
        values, labels = np.unique(np.loadtxt(os.path.join(folder, NAME + "_graph_labels.txt"), dtype=np.int64, ndmin=1), return_inverse=True)
        d = dict(graphs=[(np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)) for n in sizes.tolist()],
                 graph_labels=labels.astype(np.int64), num_labels=len(values))
    else:
        d = ingest.read_tudataset(folder, NAME)
    return d, DeviceGraphCorpus(d["graphs"], batch_size, labels=d["graph_labels"], device=tu.device, lib=tu.lib, ptr=tu.ptr, **kw)


def tables_of(corpus):
    return {k: corpus[k].cpu().numpy().copy() for k in TABLES if k in corpus}


def assert_is_host(tu, got, d, hc):
    """what TUIngestEngine.read_tudataset returned against the host-built corpus"""
    c = got["corpus"]
    assert np.array_equal(got["graph_labels"], d["graph_labels"]) and got["graph_labels"].dtype == np.int64
    assert got["num_labels"] == d["num_labels"]
    assert np.array_equal(c["sizes"], hc.sizes) and np.array_equal(c["entries"], hc.entries) and c["sizes"].dtype == np.int64
    for name in ("node_first", "row_ptr", "col_idx", "seed_local", "labels"):
        assert c[name].dtype == torch.int32 and c[name].device.type == tu.device.type
        assert np.array_equal(c[name].cpu().numpy(), getattr(hc, name).cpu().numpy()), name
    longest = int(np.diff(hc.row_ptr.cpu().numpy()).max())
    assert [int(x) for x in got["counts"]] == [len(hc.sizes), d["num_labels"], int(hc.sizes.max()), int(hc.entries.max()), longest, 0, 0, 0]


def check_case(tu, name, tmp_path):
    """files in two line orders -> the host's tables, bit for bit, by the engine and by the bare call"""
    pairs, indicator, labels = CASES[name]
    d, hc = host_corpus(tu, write_files(tmp_path / "host", pairs, indicator, labels))
    seen = []
    for seed in (11, 12):
        folder = write_files(tmp_path / f"p{seed}", pairs, indicator, labels, seed=seed, sep=", " if seed == 11 else ",")
        for _ in range(tu.calls):
            got = tu.engine.read_tudataset(folder, NAME)
            assert_is_host(tu, got, d, hc)
            seen.append(tables_of(got["corpus"]))
    # the bare call, its outputs poisoned first
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(tu.device)      # noqa: E731
    order = np.random.Generator(np.random.PCG64(13)).permutation(len(pairs))
    for _ in range(tu.calls):
        res = tu.engine.corpus(put(pairs[order].reshape(-1, 2)), put(indicator), put(labels))
        assert int(res["status"].cpu()[0]) == 0
        t = tables_of(res)
        assert np.array_equal(t["edge_first"], hc.row_ptr.cpu().numpy()[hc.first])
        seen.append({k: v for k, v in t.items() if k != "edge_first"})
    for other in seen[1:]:
        assert all(np.array_equal(other[k], seen[0][k]) for k in seen[0]), "two calls or two line orders differ"


# ---------------------------------------------------------------------------------------------------------------- errors
def _with(pairs, *more):
    return np.concatenate([pairs, np.array(more, dtype=np.int64).reshape(-1, 2)])


def _error_cases():
    pairs, indicator, labels = dataset([TRIANGLE, path(3), star(WAVE_ROW + 5)], [0, 1, 0])
    n = len(indicator)
    down = indicator.copy()
    down[4] = 1
    e = {}
    e["descends"] = (pairs, down, labels)
    e["graph_count_more_labels"] = (pairs, indicator, np.array([0, 1, 0, 1]))
    e["graph_count_fewer_labels"] = (pairs, indicator, np.array([0, 1]))
    e["id_zero"] = (_with(pairs, (0, 1)), indicator, labels)
    e["id_above_n"] = (_with(pairs, (1, n + 1), (n + 1, 1)), indicator, labels)
    e["id_negative"] = (_with(pairs, (-3, 2)), indicator, labels)
    e["self_loop"] = (_with(pairs, (2, 2)), indicator, labels)
    e["cross_graph"] = (_with(pairs, (1, 4), (4, 1)), indicator, labels)
    e["repeated"] = (_with(pairs, (1, 2), (2, 1)), indicator, labels)
    e["repeated_in_a_long_row"] = (_with(pairs, (7, 9), (9, 7)), indicator, labels)
    e["asymmetric"] = (_with(pairs, (4, 6)), indicator, labels)
    e["asymmetric_missing_line"] = (pairs[1:], indicator, labels)
    # two at once: the host's first
    e["self_loop_and_asymmetric"] = (_with(pairs, (2, 2), (4, 6)), indicator, labels)
    e["out_of_range_and_repeated"] = (_with(pairs, (1, 2), (2, 1), (n + 7, 1)), indicator, labels)
    e["cross_graph_and_repeated"] = (_with(pairs, (1, 2), (2, 1), (1, 4), (4, 1)), indicator, labels)
    e["descends_and_self_loop"] = (_with(pairs, (2, 2)), down, labels)
    e["descends_and_out_of_range"] = (_with(pairs, (n + 1, 1)), down, labels)
    e["descends_and_graph_count"] = (pairs, down, np.array([0, 1]))
    e["graph_count_and_cross_graph"] = (_with(pairs, (1, 4), (4, 1)), indicator, np.array([0, 1, 0, 1, 1]))
    return e


ERRORS = _error_cases()


def check_error(tu, name, tmp_path):
    """the host reader's ValueError, word for word, in any line order"""
    pairs, indicator, labels = ERRORS[name]
    with pytest.raises(ValueError) as host:
        ingest.read_tudataset(write_files(tmp_path / "host", pairs, indicator, labels), NAME)
    for seed in (21, 22):
        folder = write_files(tmp_path / f"p{seed}", pairs, indicator, labels, seed=seed)
        for _ in range(tu.calls):
            with pytest.raises(ValueError) as dev:
                tu.engine.read_tudataset(folder, NAME)
            assert str(dev.value) == str(host.value)
    if name.startswith("graph_count"):
        assert str(host.value) == f"3 graphs in graph_indicator but {len(labels)} graph labels"


def check_status_bits(tu):
    """the bare call's word: a step runs only on what the steps before it found sound"""
    S = _cabi
    want = {"descends": S.STATUS_TU_DESCENDS, "graph_count_more_labels": S.STATUS_TU_GRAPH_COUNT, "id_zero": S.STATUS_TU_BAD_ID,
            "self_loop": S.STATUS_TU_SELF_LOOP, "cross_graph": S.STATUS_TU_CROSS_GRAPH, "repeated": S.STATUS_TU_REPEATED,
            "repeated_in_a_long_row": S.STATUS_TU_REPEATED, "asymmetric": S.STATUS_TU_ASYMMETRIC,
            "self_loop_and_asymmetric": S.STATUS_TU_SELF_LOOP, "out_of_range_and_repeated": S.STATUS_TU_BAD_ID,
            "cross_graph_and_repeated": S.STATUS_TU_CROSS_GRAPH, "descends_and_self_loop": S.STATUS_TU_DESCENDS,
            "graph_count_and_cross_graph": S.STATUS_TU_GRAPH_COUNT}
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(tu.device)      # noqa: E731
    for name, bits in want.items():
        pairs, indicator, labels = ERRORS[name]
        for _ in range(tu.calls):
            res = tu.engine.corpus(put(pairs), put(indicator), put(labels))
            assert int(res["status"].cpu()[0]) == bits, name
            if bits == S.STATUS_TU_GRAPH_COUNT:
                assert int(res["counts"].cpu()[0]) == 3
    # a self loop and an edge between two graphs are found together
    pairs, indicator, labels = ERRORS["cross_graph"]
    res = tu.engine.corpus(put(_with(pairs, (2, 2))), put(indicator), put(labels))
    assert int(res["status"].cpu()[0]) == S.STATUS_TU_SELF_LOOP | S.STATUS_TU_CROSS_GRAPH


def check_device_only_errors(tu, tmp_path):
    """a token that is no integer, a line of the wrong shape, a value outside int32: the file and the byte offset"""
    pairs, indicator, labels = dataset([TRIANGLE, path(3)], [0, 1])

    def broken(which, old, new, count=1):
        folder = write_files(tmp_path / f"b{len(os.listdir(tmp_path))}", pairs, indicator, labels)
        path_ = os.path.join(folder, f"{NAME}_{which}.txt")
        data = open(path_, "rb").read()
        assert old in data
        at = data.index(old)
        open(path_, "wb").write(data[:at] + new + data[at + len(old):])
        return folder, path_, at

    for which, old, new, shift, pattern in (
            ("A", b"2, 1\n", b"2, x1\n", 3, "a line holds something other than integers \\(the token b'x1' at byte {at}\\)"),
            ("A", b"2, 1\n", b"2, 1_0\n", 3, "a line holds something other than integers \\(the token b'1_0' at byte {at}\\)"),
            ("A", b"2, 1\n", b"# 2, 1\n", 0, "a line holds something other than integers \\(the token b'#' at byte {at}\\)"),
            ("A", b"2, 1\n", b"2, 1, 5\n", 6, "every line must hold two integers `u, v` \\(the token b'5' at byte {at}\\)"),
            ("A", b"2, 1\n", b"2\n", 2, "every line must hold two integers `u, v` \\(the token b'[0-9]+' at byte {at}\\)"),
            ("graph_indicator", b"1\n1\n", b"1 1\n", 2, "every line must hold one integer \\(the token b'1' at byte {at}\\)"),
            ("graph_labels", b"0\n", b"0.5\n", 0, "a line holds something other than integers \\(the token b'0.5' at byte {at}\\)"),
            ("graph_labels", b"1\n", b"2147483648\n", 0, "a value does not fit int32 \\(the token b'2147483648' at byte {at}\\)"),
            ("graph_indicator", b"2\n", b"-2147483649\n", 0, "a value does not fit int32 \\(the token b'-2147483649' at byte {at}\\)")):
        folder, path_, at = broken(which, old, new)
        with pytest.raises(ValueError, match=re.escape(path_) + ": " + pattern.format(at=at + shift)):
            tu.engine.read_tudataset(folder, NAME)
    # the last line of A.txt holds one token, with and without its newline
    for tail in (b"3\n", b"3"):
        folder = write_files(tmp_path / f"t{len(tail)}", pairs, indicator, labels)
        path_ = os.path.join(folder, NAME + "_A.txt")
        size = os.path.getsize(path_)
        open(path_, "ab").write(tail)
        with pytest.raises(ValueError, match=f"every line must hold two integers `u, v` \\(the token b'3' at byte {size}\\)"):
            tu.engine.read_tudataset(folder, NAME)
    # an id of A.txt outside int32 is the host's own error, in the host's place
    folder, _, _ = broken("A", b"2, 1\n", b"2, 4294967297\n")
    with pytest.raises(ValueError, match="^node id out of range in A.txt$"):
        tu.engine.read_tudataset(folder, NAME)
    with pytest.raises(ValueError, match="^node id out of range in A.txt$"):
        ingest.read_tudataset(folder, NAME)
    # empty files
    folder = write_files(tmp_path / "empty", pairs, indicator, labels)
    open(os.path.join(folder, NAME + "_graph_labels.txt"), "w").close()
    with pytest.raises(ValueError, match="graph_labels.txt: the file holds no integer"):
        tu.engine.read_tudataset(folder, NAME)
    # the reference's dataset names map like the host reader's
    folder = write_files(tmp_path / "named", pairs, indicator, labels)
    for kind in ("A", "graph_indicator", "graph_labels"):
        os.rename(os.path.join(folder, f"{NAME}_{kind}.txt"), os.path.join(folder, f"IMDB-BINARY_{kind}.txt"))
    assert np.array_equal(tu.engine.read_tudataset(folder, "imdb-binary")["graph_labels"], ingest.read_tudataset(folder, "imdb-binary")["graph_labels"])


# ---------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(tu):
    eng, dev = tu.engine, tu.device
    pairs, indicator, labels = dataset([TRIANGLE, path(3)], [0, 1])
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(dev)            # noqa: E731
    p, ind, lab = put(pairs), put(indicator), put(labels)

    def fresh():
        out = eng._buffers(len(indicator), len(pairs), len(labels), dev)
        for k in TABLES:
            out[k].fill_(FILL)
        return out

    def untouched(out):
        assert all((out[k].cpu().numpy() == FILL).all() for k in TABLES if out[k] is not None) and int(out["status"].cpu()[0]) == 0

    for member in ("node_first", "edge_first", "row_ptr", "col_idx", "seed_local", "labels", "counts"):
        out = fresh()
        out[member] = None
        with pytest.raises(RuntimeError, match=f"gcc_tu_corpus.*{member} is NULL"):
            eng.corpus_into(p, ind, lab, len(pairs), out)
        untouched(out)
    out = fresh()
    for args, pattern in (((None, ind, lab, len(pairs)), "pairs is NULL"), ((p, None, lab, len(pairs)), "num_nodes 0 outside 1"),
                          ((p, ind, None, len(pairs)), "num_labels 0 outside 1"), ((p, ind, lab, -1), "num_lines -1 outside 0"),
                          ((p, ind, lab, 2 ** 31), "num_lines 2147483648 outside 0")):
        with pytest.raises(RuntimeError, match="gcc_tu_corpus.*" + pattern):
            eng.corpus_into(*args, out)
    with pytest.raises(RuntimeError, match="gcc_tu_corpus.*workspace_bytes 64 is less than gcc_tu_corpus_workspace_bytes"):
        eng.corpus_into(p, ind, lab, len(pairs), out, workspace_bytes=64)
    untouched(out)
    a = _cabi.GccTuCorpusArgs(pairs=tu.ptr(p), indicator=None, graph_labels=tu.ptr(lab), num_nodes=6, num_lines=len(pairs), num_labels=2)
    with pytest.raises(RuntimeError, match="gcc_tu_corpus.*status is NULL"):
        _cabi.call(tu.lib, "gcc_tu_corpus", ctypes.byref(a), tu.ptr(eng.workspace(1 << 16, dev)), 1 << 16, None, None)
    with pytest.raises(RuntimeError, match="gcc_tu_corpus.*indicator is NULL"):
        eng.invoke("gcc_tu_corpus", a, eng.workspace(1 << 16, dev), out["status"])
    q = tu.lib.gcc_tu_corpus_workspace_bytes
    assert q(0, 0, 1) < 0 and b"num_nodes 0 outside" in tu.lib.gcc_last_error()
    assert q(2 ** 31 - 1, 0, 1) < 0 and q(1, 2 ** 31, 1) < 0 and q(1, -1, 1) < 0 and q(1, 0, 0) < 0 and b"num_labels 0" in tu.lib.gcc_last_error()
    assert q(1, 0, 1) > 0 and q(2 ** 31 - 2, 2 ** 31 - 1, 5) > 0
    with pytest.raises(ValueError, match="pairs must be a contiguous int32 tensor"):
        eng.corpus(p.long(), ind, lab)
    with pytest.raises(ValueError, match="indicator must be a contiguous int32 tensor"):
        eng.corpus(p, ind.long(), lab)


def check_cpu_tensor_refused(lib, tmp_path):
    eng = TUIngestEngine(lib, _cabi.dev_ptr, "cpu")
    pairs, indicator, labels = dataset([TRIANGLE], [0])
    z = lambda a: torch.from_numpy(a.astype(np.int32))              # noqa: E731
    folder = write_files(tmp_path / "cpu", pairs, indicator, labels)
    for call in (lambda: eng.corpus(z(pairs), z(indicator), z(labels)), lambda: eng.read_tudataset(folder, NAME)):
        with pytest.raises(RuntimeError, match="device \\(HIP\\) tensors only"):
            call()


# ---------------------------------------------------------------------------------------------------------------- from_device
def generated(seed=5, graphs=37):
    """graphs of 1..40 nodes, some of them edge-free, some with isolated nodes; sparse labels"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(graphs):
        n = int(rng.integers(1, 41))
        k = int(rng.integers(0, 3 * n))
        edges = {(min(a, b), max(a, b)) for a, b in rng.integers(0, n, size=(k, 2)).tolist() if a != b}
        out.append((n, sorted(edges)))
    return dataset(out, rng.choice([-4, 0, 9, 31], size=graphs).tolist())


def check_from_device(tu, tmp_path):
    pairs, indicator, labels = generated()
    folder = write_files(tmp_path / "gen", pairs, indicator, labels, seed=31)
    d, hc = host_corpus(tu, folder, batch_size=8, pos_dim=4, expand=2)
    got = tu.engine.read_tudataset(folder, NAME)
    assert_is_host(tu, got, d, hc)
    dc = DeviceGraphCorpus.from_device(got["corpus"], 8, pos_dim=4, expand=2, device=tu.device, lib=tu.lib, ptr=tu.ptr)
    for name in ("sizes", "entries", "first"):
        assert np.array_equal(getattr(dc, name), getattr(hc, name)) and getattr(dc, name).dtype == getattr(hc, name).dtype, name
    for name in ("node_first", "row_ptr", "col_idx", "seed_local", "labels", "status", "parent_nid", "_placeholder"):
        a, b = getattr(dc, name), getattr(hc, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), name
    assert (dc.node_cap, dc.edge_cap, dc.batch_size, dc.pos_dim, dc.expand) == (hc.node_cap, hc.edge_cap, hc.batch_size, hc.pos_dim, hc.expand)
    assert dc.c.num_graphs == hc.c.num_graphs and dc.c.pos_dim == hc.c.pos_dim and dc.pos is None and len(dc._ring) == len(hc._ring)
    assert all(sorted(x) == sorted(y) and all(x[k].shape == y[k].shape and x[k].dtype == y[k].dtype for k in x) for x, y in zip(dc._ring, hc._ring))
    assert DeviceGraphCorpus.from_device(got["corpus"], 8, with_labels=False, device=tu.device, lib=tu.lib, ptr=tu.ptr).labels is None
    # one pack of a mixed index list with a padding entry
    idx = np.array([36, 0, 17, 5, 5, 30, 2], dtype=np.int64)
    pos = torch.arange(int(hc.first[-1]) * 4, dtype=torch.float32, device=tu.device).reshape(-1, 4).contiguous()
    packs = []
    for corpus in (hc, dc):
        corpus.set_pos(pos)
        for _ in range(tu.calls):
            g, lab = corpus.pack(corpus.index_tensor(idx), corpus.entries[idx].sum())
            corpus.check_status()
            packs.append([t.cpu().clone() for t in (g.node_off, g.edge_off, g.graph_id, g.row_ptr, g.col_idx, g.seed_local, g.pos_undirected, lab)])
    assert int(packs[0][-1][-1]) == -1                              # (the padding row's label)
    for other in packs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(other, packs[0]))
    with pytest.raises(ValueError, match="corpus\\['row_ptr'\\] must be a contiguous int32 tensor"):
        DeviceGraphCorpus.from_device(dict(got["corpus"], row_ptr=got["corpus"]["row_ptr"][:-1]), 8, device=tu.device, lib=tu.lib, ptr=tu.ptr)


def check_write_tudataset(tmp_path):
    """the writer is the reader's inverse, with either separator"""
    pairs, indicator, labels = generated(seed=6, graphs=9)
    d = ingest.read_tudataset(write_files(tmp_path / "a", pairs, indicator, labels), NAME)
    for sep in (", ", ","):
        paths = ingest.write_tudataset(str(tmp_path / ("w" + str(len(sep)))), NAME, d["graphs"], labels, sep=sep)
        assert [os.path.basename(p) for p in paths] == [f"{NAME}_A.txt", f"{NAME}_graph_indicator.txt", f"{NAME}_graph_labels.txt"]
        back = ingest.read_tudataset(os.path.dirname(paths[0]), NAME)
        assert np.array_equal(back["graph_labels"], d["graph_labels"]) and back["num_labels"] == d["num_labels"]
        assert len(back["graphs"]) == len(d["graphs"])
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(back["graphs"], d["graphs"]))
    with pytest.raises(ValueError, match="9 graphs but 8 graph labels"):
        ingest.write_tudataset(str(tmp_path / "bad"), NAME, d["graphs"], labels[:-1])
