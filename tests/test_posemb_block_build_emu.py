"""The sparse block class's matrix build by lane groups, its pipelined Cholesky steps and its two-node expansion on the
wave64 emulator: the smallest items that cross each boundary of the new code (tests/posemb_block_build_cases.py), against
the strict invariants of tests/test_posemb_emu.py and, bit for bit, against what the library of the commit before wrote
on this tier (tests/golden/posemb_block_build_bits_emu.npz; the change reorders work, no arithmetic operation)."""
import numpy as np
import pytest

from tests import posemb_block_build_cases as K
from tests import test_posemb_emu as T
from tests.golden.make_posemb_block_build_golden import golden_path, run

CASES = K.cases()


def check_case(tier, name, check, set_hidden):
    """status words, the strict invariants (``check``) and the recorded bits of case ``name`` on ``tier``"""
    view, hidden, handed = CASES[name]
    set_hidden(hidden)
    red = T.reduced_sizes(view)
    assert (red > 128).all(), red                                       # every item is the block class's
    x, evals, raw, status = run(tier, view, hidden)
    print(name, "deflated sizes", red.tolist(), "status", status[:5])
    assert status[0] == 0 and status[2] == 0 and status[3] == handed, status
    assert (status[1] >= 2) == (handed == 0), status                    # filter rounds: the block class solved it
    check(view, x, evals, raw)
    z = np.load(golden_path(tier))
    for key, arr in (("pos", x), ("evals", evals), ("raw", raw)):
        assert np.array_equal(K.bits(arr), z["%s_%s" % (name, key)]), (name, key)


def test_the_cases_cross_the_boundaries_they_are_named_for():
    assert T.reduced_sizes(CASES["sizes"][0]).tolist() == [129, 131]     # just above the 65..128 class, no multiple of 8 or 128
    view, special = K.row_length_item()
    keep, cnt = K.kept_rows(view)
    rp, ci = view["row_ptr"].numpy(), view["col_idx"].numpy()
    assert int(keep.sum()) == T.reduced_sizes(view)[0] and 128 < keep.sum() <= 160
    assert sorted(set(length for _, length, _ in special)) == sorted(K.ROW_LENGTHS)
    for v, length, attach in special:
        assert cnt[v] == length and rp[v + 1] - rp[v] == length + (3 if attach else 0), (v, length, attach)
        if attach and length >= 63:                                      # long rows: dropped entries between kept ones in one 8-entry round
            k8 = keep[ci[rp[v]:rp[v + 1]]]
            rounds = [np.flatnonzero(k8[r:r + 8]) for r in range(0, len(k8), 8)]
            assert any(len(w) >= 2 and w[-1] - w[0] >= len(w) for w in rounds), (v, length)
    lens = set(int(rp[v + 1] - rp[v]) for v, _, _ in special)
    assert {8, 9, 64, 65} <= lens and max(lens) > 65                     # the round boundary and the switch to the wave-wide path
    slots = set(v % 8 for v, _, _ in special)
    assert {0, 7} <= slots and len(slots) > 2                            # first and last slot of a wave's groups, and between
    # the 32-column block is tried when at most 20 pairs are wanted of the quotient (kChNarrowWant), else the 64-column one
    assert 32 - (25 - 1) <= 20 < 32 - (4 - 1)
    m = CASES["multigraph"][0]
    mrp, mci = m["row_ptr"].numpy(), m["col_idx"].numpy()
    run_len = np.diff(np.flatnonzero(np.r_[True, (np.diff(mci) != 0) | np.isin(np.arange(1, len(mci)), mrp), True]))
    assert {1, 2, 3} <= set(run_len.tolist())                            # single, doubled and tripled adjacent entries
    d = CASES["dense"][0]
    assert len(d["col_idx"]) > K.CSR_CAP and 190 <= T.reduced_sizes(d)[0] <= 210


@pytest.mark.parametrize("name", list(CASES))
def test_block_build_case_on_the_emulator(name, monkeypatch):
    check_case("emu", name, T._check, lambda h: monkeypatch.setattr(T, "HID", h))
