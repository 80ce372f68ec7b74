"""gcc_text_ints / gcc_text_line_ends and TextIngestEngine (gcc_amd/csrc/text_ingest.hip, gcc_amd/text_ingest.py) against the host
reader, shared by the emulator tier (tests/test_text_ingest_emu.py) and the GPU tier (tests/test_text_ingest_gpu.py): the same cases
and checks; only the library, the pointer function, the device and the number of calls differ (the GPU tier makes every call twice
and compares the bits).

The yardstick for ``ints`` is ``np.array(data[first:].split()[:max_tokens], dtype=np.int64)`` reshaped and cut to ``keep`` columns;
where a text holds tokens that NumPy cannot convert, ``model`` restates the token rule with a regular expression (and is itself
held against the yardstick on every text NumPy can convert).  The yardstick for ``read_lscc`` is ``ingest.read_lscc`` on the same
bytes in a file.  Equality is exact everywhere.  Texts come from ``make_text``, a seeded generator.

The shapes come from the constants the library exports: a tile of T = TEXT_TILE_BYTES bytes, a lane's span of 16, a wave's of 1,024,
and S = TEXT_SCAN_TILES tiles per pass of the scan.  The text of S + 1 tiles takes about a second on the emulator, so it runs in
both tiers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gcc_amd import _cabi, ingest
from gcc_amd.text_ingest import TextIngestEngine, padded

T, S = _cabi.TEXT_TILE_BYTES, _cabi.TEXT_SCAN_TILES
LANE, WAVE = 16, 1024
NOT_INT, RANGE, SHORT = _cabi.STATUS_TEXT_NOT_INTEGER, _cabi.STATUS_TEXT_INT32_RANGE, _cabi.STATUS_TEXT_SHORT
GUARD, FILL, G = 0x6B6B6B6B, 0x5A5A5A5A, 8
SEPS = np.frombuffer(b"\t\n\x0b\x0c\r ", dtype=np.uint8)
TOKEN = re.compile(rb"[^\t\n\x0b\x0c\r ]+")
INTEGER = re.compile(rb"[+-]?[0-9]+")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_FILES = ("x2dgl_tie.lscc", "x2dgl_hub.lscc", "x2dgl_small.lscc")


def make_text(nbytes, seed, max_digits=6):
    """``nbytes`` of tokens of 1..max_digits digits, one or two of the six separators between them (the text is cut where it is
    cut: it may end inside a token)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    count = nbytes // 2 + 2
    digits, gaps = rng.integers(1, max_digits + 1, size=count), rng.integers(1, 3, size=count)
    ends = np.cumsum(digits + gaps)                                 # one past a token's separators
    buf = rng.integers(48, 58, size=int(ends[-1]), dtype=np.uint8)
    buf[ends - 1] = SEPS[rng.integers(0, 6, size=count)]
    two = gaps == 2
    buf[ends[two] - 2] = SEPS[rng.integers(0, 6, size=int(two.sum()))]
    return buf[:nbytes].copy()


def put(buf, at, token):
    """``token`` at offset ``at``, a space on both sides (the tokens it cuts stay digits)"""
    token = np.frombuffer(token, dtype=np.uint8)
    if at > 0:
        buf[at - 1] = 32
    buf[at:at + len(token)] = token
    if at + len(token) < len(buf):
        buf[at + len(token)] = 32
    return buf


def yardstick(data, first, max_tokens, fields, keep):
    """the host reader's own conversion -> (records [., keep] of the complete records, the tokens found)"""
    tokens = bytes(data[first:]).split()
    vals = np.array(tokens[:max_tokens], dtype=np.int64)
    whole = len(vals) // fields * fields
    return vals[:whole].reshape(-1, fields)[:, :keep], len(tokens)


def model(data, first, max_tokens, fields, keep):
    """the token rule restated -> (flat expected words with FILL where nothing is stored, summary [4], status)"""
    data = bytes(data)
    words = np.full(max_tokens // fields * keep, FILL, dtype=np.int64)
    bad, out_of_range, r = [], [], -1
    for r, mt in enumerate(TOKEN.finditer(data, first)):
        if r >= max_tokens:
            continue
        ok = INTEGER.fullmatch(mt.group()) is not None
        if not ok:
            bad.append(mt.start())
        if r % fields < keep:
            v = int(mt.group()) if ok else 0
            if not -2 ** 31 <= v < 2 ** 31:
                out_of_range.append(mt.start())
                v = 0
            words[r // fields * keep + r % fields] = v
    total = r + 1
    status = (NOT_INT if bad else 0) | (RANGE if out_of_range else 0) | (SHORT if total < max_tokens else 0)
    return words, [total, min(bad, default=-1), min(out_of_range, default=-1), 0], status


class Ti:
    """the library under test, its pointer function and its device (the emulator works on CPU tensors); ``calls``: how often every
    call is made (their bits must agree)"""

    def __init__(self, lib, ptr, device, calls=1):
        self.lib, self.ptr, self.device, self.calls = lib, ptr, torch.device(device), calls
        self.engine = TextIngestEngine(lib, ptr, device)

    def upload(self, data):
        """the text with its padding poisoned by digits: what lies at and above nbytes must not matter"""
        text, nbytes = self.engine.upload(np.asarray(data, dtype=np.uint8) if not isinstance(data, bytes) else data)
        assert text.numel() == padded(nbytes) and text.dtype == torch.uint8
        text[nbytes:] = ord("7")
        return text, nbytes

    def ints(self, data, first, max_tokens, fields, keep):
        """the bare call into a guarded, pre-filled buffer -> (the words as int64 [.], summary as a list, status)"""
        text, nbytes = self.upload(data)
        words = max_tokens // fields * keep
        seen = []
        for _ in range(self.calls):
            out = torch.full((words + 2 * G,), FILL, dtype=torch.int32, device=self.device)
            out[:G] = GUARD
            out[G + words:] = GUARD
            summary = torch.full((4,), -7, dtype=torch.int64, device=self.device)
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.engine.ints_into(text, nbytes, first, max_tokens, fields, keep, out[G:G + words], summary, status)
            o = out.cpu().numpy()
            assert (o[:G] == GUARD).all() and (o[G + words:] == GUARD).all(), "a guard word was written"
            seen.append((o[G:G + words].astype(np.int64), [int(x) for x in summary.cpu()], int(status.cpu()[0])))
        for other in seen[1:]:
            assert np.array_equal(other[0], seen[0][0]) and other[1:] == seen[0][1:], "two calls differ"
        return seen[0]

    def line_ends(self, data, lines):
        text, nbytes = self.upload(data)
        seen = [[int(x) for x in self.engine.line_ends(text, nbytes, lines).cpu()] for _ in range(self.calls)]
        assert all(s == seen[0] for s in seen), "two calls differ"
        return seen[0]

    def read_lscc(self, source):
        seen = []
        for _ in range(self.calls):
            n, pairs = self.engine.read_lscc(source)
            assert pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2 and pairs.device.type == self.device.type
            seen.append((n, pairs.cpu().numpy()))
        assert all(s[0] == seen[0][0] and np.array_equal(s[1], seen[0][1]) for s in seen), "two calls differ"
        return seen[0]


def check_ints(ti, data, first, max_tokens, fields, keep, use_model=True, convertible=True):
    """a text against the yardstick (where NumPy converts it) and the restated rule -> (words, summary, status)"""
    data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, bytes) else data
    words, summary, status = ti.ints(data, first, max_tokens, fields, keep)
    if convertible:
        recs, total = yardstick(data, first, max_tokens, fields, keep)
        assert summary[0] == total
        got = words.reshape(-1, keep)
        assert np.array_equal(got[:len(recs)], recs), "the complete records differ from the host reader's"
        if total >= max_tokens:
            assert len(recs) == max_tokens // fields and summary[1:] == [-1, -1, 0]
    if use_model:
        m_words, m_summary, m_status = model(data, first, max_tokens, fields, keep)
        assert np.array_equal(words, m_words) and summary == m_summary and status == m_status, (summary, m_summary, status, m_status)
    return words, summary, status


# ---------------------------------------------------------------------------------------------------------------- seams
def seam_cases():
    """name -> (text, first_byte): two or three tiles, a body of a few hundred tokens around the seam"""
    c = {}
    first = T - 600

    def two_tiles(seed):
        return make_text(2 * T + 37, seed)

    c["token_straddles_a_tile"] = (put(two_tiles(1), T - 3, b"123456"), first)
    c["token_on_a_tiles_first_byte"] = (put(two_tiles(2), T, b"4321"), first)
    c["token_ends_on_a_tiles_last_byte"] = (put(two_tiles(3), T - 4, b"9876"), first)
    c["token_straddles_a_lane"] = (put(two_tiles(4), T + 5 * LANE - 2, b"2468"), first)
    c["token_on_a_lanes_first_byte"] = (put(two_tiles(5), T + 7 * LANE, b"13579"), first)
    c["token_straddles_a_wave"] = (put(two_tiles(6), T + WAVE - 2, b"8642"), first)
    c["token_on_a_waves_first_byte"] = (put(two_tiles(7), T + 2 * WAVE, b"97531"), first)
    c["token_runs_past_the_halo"] = (put(two_tiles(8), T - 5, b"0" * 40 + b"7"), first)
    c["token_runs_over_a_whole_tile"] = (put(make_text(3 * T + 5, 9), T - 9, b"0" * (T + 20) + b"12"), first)
    c["single_digits_one_space"] = (np.frombuffer(b"7 " * (T + 100), dtype=np.uint8).copy(), T - 500)      # eight starts in a lane
    return c


SEAMS = seam_cases()
FIRST_BYTES = (0, 1, 15, 16, 17, T - 1)
LENGTHS = ("T-1", "T", "T+1", "inside_a_token")


def check_seam(ti, name):
    data, first = SEAMS[name]
    total = len(bytes(data[first:]).split())
    for fields, keep in ((3, 2), (1, 1)):
        check_ints(ti, data, first, total // fields * fields, fields, keep)


def check_first_byte(ti, first):
    """first_byte inside a token, on a token's first byte and on a separator: the cut token is a token of its own"""
    for seed in (20, 21, 22):
        data = make_text(T + 300, seed)
        total = len(bytes(data[first:]).split())
        check_ints(ti, data, first, total // 3 * 3, 3, 2)
    data = put(make_text(T + 300, 23), max(first - 2, 0), b"556677")          # first_byte inside 556677 (or on its first byte)
    check_ints(ti, data, first, len(bytes(data[first:]).split()) // 2 * 2, 2, 2)


def check_length(ti, which):
    nbytes = {"T-1": T - 1, "T": T, "T+1": T + 1, "inside_a_token": T + 700}[which]
    data = make_text(nbytes, 30 + len(which))
    put(data, nbytes - 3, b"815")                                            # the text ends inside a token: no final newline
    assert data[-1] == ord("5") and len(data) == nbytes
    total = len(bytes(data).split())
    for first in (0, nbytes - 2, nbytes):
        left = len(bytes(data[first:]).split())
        check_ints(ti, data, first, left, 1, 1)
    check_ints(ti, data, 0, total // 3 * 3, 3, 2)


def check_scan_second_pass(ti):
    """S + 1 tiles: the scan's second pass, and offsets past a pass's end (the yardstick alone: the restated rule is a Python loop)"""
    data = make_text(S * T + 100, 40)
    first = 5
    total = len(bytes(data[first:]).split())
    words, summary, status = check_ints(ti, data, first, total // 3 * 3, 3, 2, use_model=False)
    assert status == 0 and summary == [total, -1, -1, 0]
    nl = np.flatnonzero(data == 10)
    at = int(np.searchsorted(nl, S * T))                                     # the first line that ends in the last tile
    assert at < len(nl)
    assert ti.line_ends(data, [0, at, len(nl) - 1, len(nl)]) == [int(nl[0]), int(nl[at]), int(nl[-1]), -1, len(nl)]


# ---------------------------------------------------------------------------------------------------------------- token forms
def check_token_forms(ti):
    words, summary, status = check_ints(ti, b"+5 -7 -0 00012 2147483647 -2147483648 +0 -00 0000000000000000000000000000001", 0, 9, 1, 1)
    assert words.tolist() == [5, -7, 0, 12, 2147483647, -2147483648, 0, 0, 1] and status == 0
    for token in (b"2147483648", b"-2147483649", b"1234567890123456789012345", b"-1234567890123456789012345", b"4294967296",
                  b"18446744073709551617", b"+99999999999"):
        text = b"1 2 " + token + b" 4\n"
        convertible = len(token) < 19
        words, summary, status = check_ints(ti, text, 0, 4, 2, 2, convertible=False)
        assert status == RANGE and summary == [4, -1, 4, 0] and words.tolist() == [1, 2, 0, 4], token
        # the same value in a dropped field sets nothing
        words, summary, status = check_ints(ti, text, 0, 4, 4, 2, convertible=convertible)
        assert status == 0 and summary == [4, -1, -1, 0] and words.tolist() == [1, 2], token
        words, summary, status = check_ints(ti, text, 0, 4, 2, 1, convertible=False)
        assert status == RANGE and summary[2] == 4, token                    # (field 0 of the second record is kept)
    words, summary, status = check_ints(ti, b"1 2147483648 2 9999999999999999999999999 3 -2147483649", 0, 6, 2, 1, convertible=False)
    assert status == 0 and summary == [6, -1, -1, 0] and words.tolist() == [1, 2, 3]
    # the lowest of two tokens out of range
    words, summary, status = check_ints(ti, b"7 -3000000000 3000000000", 0, 3, 1, 1, convertible=False)
    assert status == RANGE and summary[2] == 2


def check_separators(ti):
    text = b"  \t 1\r\n2\x0b3\x0c4     5\n\n\n6\t\t7 \r\n\r\n 8\n"
    words, summary, status = check_ints(ti, text, 0, 8, 2, 2)
    assert words.tolist() == [1, 2, 3, 4, 5, 6, 7, 8] and status == 0 and summary == [8, -1, -1, 0]
    # bytes that are NOT separators: 0, 8, 14, 28..31, 133, 160
    for c in (0, 8, 14, 28, 31, 133, 160):
        text = b"1 2" + bytes([c]) + b"3 4"
        words, summary, status = check_ints(ti, text, 0, 3, 1, 1, convertible=False)
        assert status == NOT_INT and summary == [3, 2, -1, 0], c


BAD_TOKENS = (b"x", b"3x", b"-", b"+", b"1.0", b"1_0", b"\xe9", b"12\xff", b"--1", b"+-1", b"1-", b"0x10", b"1e3")


def check_bad_token(ti, token):
    """exactly the not-integer bit and the token's own offset, kept field or dropped"""
    text = b"10 20 " + token + b" 40 50 60\n"
    for fields, keep in ((3, 2), (3, 3), (1, 1)):
        words, summary, status = check_ints(ti, text, 0, 6, fields, keep, convertible=False)
        assert status == NOT_INT and summary == [6, 6, -1, 0], (token, fields, keep)
    # as the text's last token, without a separator behind it
    text = b"10 20 " + token
    words, summary, status = check_ints(ti, text, 0, 3, 1, 1, convertible=False)
    assert status == NOT_INT and summary == [3, 6, -1, 0], token


def check_lowest_bad_token(ti):
    """three bad tokens in three tiles: the lowest offset, in whatever order the workgroups run; one after max_tokens sets nothing"""
    data = make_text(3 * T, 50)
    for at, token in ((2 * T + 77, b"3x"), (T - 2, b"1.0"), (T + 900, b"-")):
        put(data, at, token)
    total = len(bytes(data).split())
    words, summary, status = check_ints(ti, data, 0, total, 1, 1, convertible=False)
    assert status == NOT_INT and summary[1] == T - 2
    before = len(bytes(data[:T - 2]).split())                               # the tokens before the first bad one
    words, summary, status = check_ints(ti, data, 0, before, 1, 1, convertible=False)
    assert status == 0 and summary == [total, -1, -1, 0]
    words, summary, status = check_ints(ti, data, 0, before + 1, 1, 1, convertible=False)
    assert status == NOT_INT and summary[1] == T - 2
    # a bad token and one out of range: both bits, both offsets
    put(data, 40, b"5000000000")
    words, summary, status = check_ints(ti, data, 0, total, 1, 1, convertible=False)
    assert status == NOT_INT | RANGE and summary[1:3] == [T - 2, 40]


def check_counts(ti):
    data = make_text(T + 500, 60)
    total = len(bytes(data).split())
    for fields, keep in ((3, 2), (2, 2), (1, 1), (4, 1), (4, 4), (4, 3)):
        whole = total // fields * fields
        words, summary, status = check_ints(ti, data, 0, whole, fields, keep)
        assert status == 0
        words, summary, status = check_ints(ti, data, 0, whole + 2 * fields, fields, keep)          # more announced than there are
        assert status == SHORT and summary == [total, -1, -1, 0]
        words, summary, status = check_ints(ti, data, 0, fields, fields, keep)                      # one record of a long text
        assert status == 0 and summary[0] == total
    # an empty body, and nothing asked for
    for first, max_tokens in ((len(data), 0), (len(data), 3), (0, 0)):
        words, summary, status = check_ints(ti, data, first, max_tokens, 3, 2)
        assert status == (SHORT if max_tokens else 0) and summary[0] == (0 if first else total)
    words, summary, status = check_ints(ti, b" \n\t \r\n", 0, 2, 2, 2)
    assert status == SHORT and summary == [0, -1, -1, 0]
    words, summary, status = check_ints(ti, b"5", 0, 1, 1, 1)
    assert status == 0 and words.tolist() == [5]


# ---------------------------------------------------------------------------------------------------------------- line ends
def check_line_ends(ti):
    data = make_text(3 * T + 123, 70)
    data[data == 10] = 32
    for at in (7, T - 1, 2 * T, 2 * T + 1, 2 * T + 500, 3 * T + 100):        # a tile's last byte, a tile's first byte, neighbours
        data[at] = 10
    nl = np.flatnonzero(data == 10)
    assert nl.tolist() == [7, T - 1, 2 * T, 2 * T + 1, 2 * T + 500, 3 * T + 100]
    assert ti.line_ends(data, [0, 1, 2, 5, 6]) == [7, T - 1, 2 * T, 3 * T + 100, -1, 6]
    assert ti.line_ends(data, [6, 3, 3, 0, 2 ** 40]) == [-1, 2 * T + 1, 2 * T + 1, 7, -1, 6]       # any order, repeats
    assert ti.line_ends(data, []) == [6]
    assert ti.line_ends(data, list(range(16))) == nl.tolist() + [-1] * 10 + [6]
    # every newline of a generated text, sixteen at a time
    data = make_text(T + 50, 71)
    nl = np.flatnonzero(data == 10)
    for at in range(0, len(nl), 16):
        lines = list(range(at, min(at + 16, len(nl))))
        assert ti.line_ends(data, lines) == nl[lines].tolist() + [len(nl)]
    # a newline as the text's last byte, and a text without any
    assert ti.line_ends(b"ab\ncd\n", [0, 1, 2]) == [2, 5, -1, 2]
    assert ti.line_ends(b"no newline in here", [0, 1]) == [-1, -1, 0]
    assert ti.line_ends(b"\n", [0, 1]) == [0, -1, 1]


# ---------------------------------------------------------------------------------------------------------------- read_lscc
def lscc_text(n, m, seed):
    """the layout read_lscc takes: n vertex lines, m lines ``u v w`` with repeats and self loops"""
    rng = np.random.Generator(np.random.PCG64(seed))
    uv = rng.integers(0, n, size=(m, 2))
    lines = [f"vertices {n}\n"] + [f"{i} {1000 + i}\n" for i in range(n)] + [f"edges {m}\n"]
    lines += [f"{u} {v} 1\n" for u, v in uv]
    return "".join(lines).encode()


LSCC_SIZES = (1, T // 4, 2 * T)


def check_read_lscc_file(ti, path):
    n, pairs = ingest.read_lscc(str(path))
    got_n, got = ti.read_lscc(str(path))
    assert got_n == n and got.dtype == pairs.dtype and np.array_equal(got, pairs)
    with open(path, "rb") as f:                                              # the same text as bytes
        data = f.read()
    got_n, got = ti.read_lscc(data)
    assert got_n == n and np.array_equal(got, pairs)


def check_read_lscc_generated(ti, n, tmp_path):
    path = tmp_path / f"n{n}.lscc"
    path.write_bytes(lscc_text(n, 300, n))
    check_read_lscc_file(ti, path)


def check_read_lscc_errors(ti, tmp_path):
    """tests/test_x2dgl_task.py's three truncations and its ``3 x 1`` line, against the host reader's own messages"""
    text = open(os.path.join(GOLDEN, "x2dgl_small.lscc")).read().splitlines(keepends=True)
    cut = tmp_path / "cut.lscc"

    def both(content, pattern, same_text=True):
        cut.write_bytes(content if isinstance(content, bytes) else content.encode())
        with pytest.raises(ValueError, match=pattern) as host:
            ingest.read_lscc(str(cut))
        with pytest.raises(ValueError, match=pattern) as dev:
            ti.engine.read_lscc(str(cut))
        if same_text:
            assert str(dev.value) == str(host.value)

    both("".join(text[:-2]), "cut.lscc: truncated: 11 edge lines `u v w` announced, 9 complete ones found")
    both("".join(text[:5]), "cut.lscc: truncated: 9 vertex lines and a `<word> m` line announced, the file has 5 lines")
    both("".join(text[:-1]) + "3 x 1\n", "cut.lscc: an edge line holds something other than integers", same_text=False)
    with pytest.raises(ValueError, match=r"other than integers \(the token b'x' at byte \d+\)"):
        ti.engine.read_lscc(str(cut))
    both("vertices 3", "cut.lscc: truncated: no `<word> n` line")
    both("", "cut.lscc: truncated: no `<word> n` line")
    both("vertices\n0 0\n", "cut.lscc: expected a `<word> n` line, found b'vertices'")
    both("vertices 1\n0 7\nedges many\n0 0 1\n", "cut.lscc: expected a `<word> m` line, found b'edges many'")
    both("vertices -1\n0 7\nedges 1\n0 0 1\n", "cut.lscc: truncated: -1 vertex lines and a `<word> m` line announced, the file has 4 lines")
    both("vertices 1\n0 7\nedges -2\n0 0 1\n", "cut.lscc: truncated: -2 edge lines `u v w` announced, 1 complete ones found")
    both(f"vertices 1\n0 7\nedges 2\n0 0 1\n0 {2 ** 31} 1\n", "cut.lscc: node ids must fit int32")
    both(f"vertices 1\n0 7\nedges 1\n{-2 ** 31 - 1} 0 1\n", "cut.lscc: node ids must fit int32")
    # what the host reader would take: w outside int32, ids at the edges of int32, a last line without its newline, m = 0
    for content in (f"vertices 1\n0 7\nedges 2\n0 0 {2 ** 40}\n{2 ** 31 - 1} {-2 ** 31} 1", "v 0\ne 0\n", "v 2\n0 5\n1 6\ne 1\n\n\n 0\t1\r\n1\n"):
        cut.write_bytes(content.encode())
        check_read_lscc_file(ti, cut)
    # the first documented difference: what follows the 3 m-th token is not looked at
    cut.write_text("vertices 1\n0 7\nedges 1\n0 0 1\nrubbish\n")
    with pytest.raises(ValueError, match="other than integers"):
        ingest.read_lscc(str(cut))
    assert ti.read_lscc(str(cut))[1].tolist() == [[0, 0]]
    # the second: an underscore is no digit
    cut.write_text("vertices 1\n0 7\nedges 1\n0 1_0 1\n")
    assert ingest.read_lscc(str(cut))[1].tolist() == [[0, 10]]
    with pytest.raises(ValueError, match=r"other than integers \(the token b'1_0' at byte"):
        ti.engine.read_lscc(str(cut))


# ---------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(ti):
    eng, dev = ti.engine, ti.device
    text, nbytes = ti.upload(make_text(100, 80))
    out = torch.full((64,), FILL, dtype=torch.int32, device=dev)
    summary = torch.full((4,), -7, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def ints(nbytes=nbytes, first=0, max_tokens=6, fields=3, keep=2, text=text, out=out, summary=summary, status=status, **kw):
        eng.ints_into(text, nbytes, first, max_tokens, fields, keep, out, summary, status, **kw)

    for kw, pattern in ((dict(nbytes=0), "nbytes 0 outside 1"), (dict(nbytes=-3), "nbytes -3 outside 1"),
                        (dict(first=-1), "first_byte -1 outside \\[0, nbytes = 100\\]"), (dict(first=101), "first_byte 101 outside"),
                        (dict(max_tokens=7), "max_tokens 7 is not a multiple of fields 3"), (dict(max_tokens=-3), "max_tokens -3"),
                        (dict(max_tokens=3 * 2 ** 30, keep=2), "must stay below 2\\^31"), (dict(max_tokens=2 ** 31, fields=1, keep=1), "must stay below 2\\^31"),
                        (dict(max_tokens=2 ** 62, fields=4, keep=4), "must stay below 2\\^31"),
                        (dict(fields=0), "fields 0 / keep 2"), (dict(fields=5, max_tokens=5), "fields 5 / keep 2"), (dict(keep=0), "fields 3 / keep 0"),
                        (dict(keep=4), "fields 3 / keep 4"), (dict(capacity=96), "capacity 96 is less than nbytes 100 rounded up to 16 \\(112\\)"),
                        (dict(capacity=111), "capacity 111 is less than"), (dict(workspace_bytes=64), "workspace_bytes 64 is less than gcc_text_ints_workspace_bytes"),
                        (dict(out=None), "out is NULL"), (dict(summary=None), "summary is NULL"), (dict(text=None, capacity=112), "text is NULL")):
        with pytest.raises(RuntimeError, match="gcc_text_ints.*" + pattern):
            ints(**kw)
    with pytest.raises(RuntimeError, match="gcc_text_ints.*text must be aligned to 16 bytes"):
        ints(text=text[1:], nbytes=50)
    with pytest.raises(RuntimeError, match="gcc_text_ints.*status is NULL"):
        a = _cabi.GccTextIntsArgs(text=ti.ptr(text), nbytes=nbytes, capacity=112, max_tokens=6, fields=3, keep=2, out=ti.ptr(out), summary=ti.ptr(summary))
        _cabi.call(ti.lib, "gcc_text_ints", ctypes.byref(a), ti.ptr(eng.workspace(1 << 12, dev)), 1 << 12, None, None)
    # line ends
    with pytest.raises(RuntimeError, match="gcc_text_line_ends.*num_lines 17 outside 0..16"):
        eng.line_ends(text, nbytes, list(range(17)))
    with pytest.raises(RuntimeError, match="gcc_text_line_ends.*nbytes 0 outside"):
        eng.line_ends(text, 0, [0])
    with pytest.raises(RuntimeError, match="gcc_text_line_ends.*capacity 112 is less than nbytes 113"):
        eng.line_ends(text, 113, [0])
    with pytest.raises(RuntimeError, match="workspace_bytes 8 is less than gcc_text_line_ends_workspace_bytes"):
        eng.line_ends(text, nbytes, [0], workspace_bytes=8)
    ends = torch.zeros(2, dtype=torch.int64, device=dev)
    for member, pattern in (("text", "text is NULL"), ("ends", "ends is NULL"), ("lines", "lines is NULL")):
        a = _cabi.GccTextLineEndsArgs(text=ti.ptr(text), nbytes=nbytes, capacity=112, lines=(ctypes.c_int64 * 1)(0), num_lines=1, ends=ti.ptr(ends))
        setattr(a, member, None)
        with pytest.raises(RuntimeError, match="gcc_text_line_ends.*" + pattern):
            eng.invoke("gcc_text_line_ends", a, eng.workspace(1 << 12, dev), status)
    for name in ("gcc_text_ints_workspace_bytes", "gcc_text_line_ends_workspace_bytes"):
        assert getattr(ti.lib, name)(0) < 0 and b"outside 1..2^40" in ti.lib.gcc_last_error()
        assert getattr(ti.lib, name)(2 ** 40 + 1) < 0
        assert getattr(ti.lib, name)(1) > 0 and getattr(ti.lib, name)(2 ** 40) > 0
    # nothing was launched by a refused call
    assert int(status.cpu()[0]) == 0 and (summary.cpu().numpy() == -7).all() and (out.cpu().numpy() == FILL).all() and (ends.cpu().numpy() == 0).all()
    with pytest.raises(ValueError, match="contiguous one-dimensional uint8"):
        eng.ints(text.to(torch.int32), nbytes, 0, 6, 3, 2)
    ints(max_tokens=0, out=None)                                             # (nothing to store: out may be NULL)
    assert int(summary.cpu()[0]) == len(bytes(text[:nbytes].cpu().numpy()).split()) and int(status.cpu()[0]) == 0


def check_cpu_tensor_refused(lib, tmp_path):
    eng = TextIngestEngine(lib, _cabi.dev_ptr, "cpu")
    for call in (lambda: eng.upload(b"1 2 3\n"), lambda: eng.read_lscc(b"v 0\ne 0\n"),
                 lambda: eng.ints(torch.zeros(16, dtype=torch.uint8), 5, 0, 3, 3, 2), lambda: eng.line_ends(torch.zeros(16, dtype=torch.uint8), 5, [0])):
        with pytest.raises(RuntimeError, match="device \\(HIP\\) tensors only"):
            call()
    from gcc_amd import corpus

    path = tmp_path / "g.lscc"
    path.write_text("v 2\n0 5\n1 6\ne 1\n0 1 1\n")
    with pytest.raises(ValueError, match="parse='device' needs a device"):
        corpus.build_graph(str(path), device="cpu", parse="device")
    with pytest.raises(ValueError, match="parse='device' needs a device"):
        corpus.build_corpus(str(tmp_path), ["g.lscc"], device="cpu", parse="device")
    with pytest.raises(ValueError, match="parse 'gpu'"):
        corpus.build_graph(str(path), device="cpu", parse="gpu")


# ---------------------------------------------------------------------------------------------------------------- upload
def check_upload(ti, tmp_path):
    """files around the chunk size: the tensor holds the file's bytes, then zeros up to the padded capacity"""
    rng = np.random.Generator(np.random.PCG64(90))
    for size in (63, 64, 65, 129, 0, 1, 16):
        data = rng.integers(1, 256, size=size, dtype=np.uint8)
        path = tmp_path / f"f{size}.txt"
        path.write_bytes(data.tobytes())
        want = np.concatenate([data, np.zeros(padded(size) - size, dtype=np.uint8)])
        for source in (str(path), path, data.tobytes(), data):
            text, nbytes = ti.engine.upload(source, chunk_bytes=64)
            assert nbytes == size and text.dtype == torch.uint8 and text.device.type == ti.device.type
            assert np.array_equal(text.cpu().numpy(), want), (size, type(source))
    assert padded(0) == 16 and padded(16) == 16 and padded(17) == 32
    with pytest.raises(ValueError, match="chunk_bytes 0"):
        ti.engine.upload(b"1", chunk_bytes=0)
    with pytest.raises(ValueError, match="one-dimensional uint8"):
        ti.engine.upload(np.zeros(4, dtype=np.int32))
