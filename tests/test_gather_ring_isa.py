"""The ring of row requests in the neighbour gather, read off the gfx950 listing (no GPU): in the steady-state loop of
gather_tile (gcc_amd/csrc/encoder_common.h) a row is summed behind ``s_waitcnt vmcnt(k)`` with k >= 3 -- the other half of the
ring, at least, stays in flight -- in every kernel that gathers; and gin_in_kernel keeps no scratch.  The compiler re-serialises
this loop easily (a branch around a request is enough: the comments in gather_tile), and only the listing shows it."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_chains  # noqa: E402

needs_hipcc = pytest.mark.skipif(not os.path.exists(isa_chains.HIPCC) or shutil.which("make") is None,
                                 reason="hipcc not installed")

CSRC = isa_chains.ROOT / "gcc_amd" / "csrc"
KERNELS = [("encoder.hip", "gin_in_kernel"), ("encoder_bwd.hip", "gin_bwd_c_kernel"), ("encoder_bwd.hip", "gin_bwd_emb_kernel")]
_LISTINGS = {}


def _body(src, kernel):
    if src not in _LISTINGS:
        _LISTINGS[src] = isa_chains.isa_of(CSRC / src)
    found = [b for n, b in isa_chains.kernels(_LISTINGS[src]) if re.search(r"\d+%s[A-Z]" % kernel, n)]
    assert len(found) == 1, (kernel, len(found))
    return found[0]


def loops(body):
    """loop header label -> (depth, instruction lines of the blocks that belong to this loop and to no loop inside it)"""
    out, cur = {}, None
    for s in body:
        m = re.match(r"^(\.LBB\d+_\d+):\s*;\s*(.*)$", s)
        if m:
            label, note = m.groups()
            own = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", note)
            head = re.search(r"Loop Header: Depth=(\d+)", note)
            if own:
                cur = "." + "L" + own.group(1)
                out.setdefault(cur, [int(own.group(2)), []])
            elif head:                                   # an outermost loop's header
                cur = label
                out.setdefault(cur, [int(head.group(1)), []])
            elif "Parent Loop" in note:                  # an inner loop's header: its own depth follows on a comment line
                cur = label
            else:
                cur = None
            continue
        m = re.match(r"^;\s*=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", s)
        if m and cur is not None:
            out.setdefault(cur, [int(m.group(1)), []])
            continue
        if re.match(r"^\.LBB\d+_\d+:", s):               # a label without a note: outside every loop
            cur = None
            continue
        if cur in out and s and not s.startswith((";", ".")):
            out[cur][1].append(s)
    return out


def ring_loops(body):
    """the gather's steady-state loops: inside the tile loop, two halves of four row requests per trip (gin_bwd_emb_kernel has
    two gathers: 16 bytes a lane and, at up to 16 embedding columns, 4 bytes a lane)"""
    return [ins for d, ins in loops(body).values()
            if d >= 2 and sum(i.startswith("global_load_dword") for i in ins) >= 8]


def test_loop_reader_on_a_toy_listing():
    body = [".LBB0_1:                       ; =>This Loop Header: Depth=1", "s_nop 0",
            ".LBB0_2:                       ;   Parent Loop BB0_1 Depth=1", ";     =>  This Inner Loop Header: Depth=2",
            "global_load_dwordx4 v[0:3], v[4:5], off", "s_waitcnt vmcnt(4)",
            ".LBB0_3:                       ;   in Loop: Header=BB0_2 Depth=2", "s_waitcnt vmcnt(5)",
            ".LBB0_4:                       ;   in Loop: Header=BB0_1 Depth=1", "s_waitcnt vmcnt(0)"]
    got = loops(body)
    assert got[".LBB0_2"] == [2, ["global_load_dwordx4 v[0:3], v[4:5], off", "s_waitcnt vmcnt(4)", "s_waitcnt vmcnt(5)"]]
    assert got[".LBB0_1"][1] == ["s_nop 0", "s_waitcnt vmcnt(0)"]


@needs_hipcc
@pytest.mark.parametrize("src,kernel", KERNELS)
def test_steady_state_sums_rows_with_the_other_half_in_flight(src, kernel):
    found = ring_loops(_body(src, kernel))
    assert len(found) == (2 if kernel == "gin_bwd_emb_kernel" else 1), (kernel, len(found))
    for ins in found:
        waits = [int(m.group(1)) for i in ins for m in [re.search(r"s_waitcnt.*vmcnt\((\d+)\)", i)] if m]
        print(kernel, "vmcnt in the ring loop:", waits)
        assert len(waits) >= 8, (kernel, waits)          # a wait in front of every row of both halves
        assert min(waits) >= 3, (kernel, waits)


@needs_hipcc
def test_gin_in_keeps_no_scratch():
    md = isa_chains.metadata(_LISTINGS.get("encoder.hip") or isa_chains.isa_of(CSRC / "encoder.hip"), "gin_in_kernel")
    assert md["private_segment_fixed_size"] == 0, md
    assert md.get("vgpr_spill_count", 0) == 0, md
