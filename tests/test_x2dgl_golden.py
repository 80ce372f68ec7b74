"""The converter's rule against the reference's own function: tests/golden/x2dgl_golden.npz holds what
``yuxiao_kdd17_graph_to_dgl`` made of the three files tests/golden/x2dgl_*.lscc (tests/golden/make_x2dgl_golden.py).  Both the NumPy
restatement and the kernels on the emulator reproduce its CSR and the four numbers of its log line exactly."""
import os

import numpy as np
import pytest

from gcc_amd import ingest
from gcc_amd.graph_build import GraphBuildEngine, build_csr_numpy

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("small", "tie", "hub")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "x2dgl_golden.npz")))


def agrees(out, golden, name):
    assert np.array_equal(out["row_ptr"], golden[f"{name}_row_ptr"]) and np.array_equal(out["col_idx"], golden[f"{name}_col_idx"])
    nodes, edges, loop_slots, removed = (int(x) for x in golden[f"{name}_log"])
    counts = [int(c) for c in out["counts"]]
    assert (counts[0], counts[1], 2 * counts[2], counts[4]) == (nodes, edges, loop_slots, removed)
    assert int(out["status"][0]) == 0


@pytest.mark.parametrize("name", NAMES)
def test_file_reader_returns_the_lines_as_written(golden, name):
    n, pairs = ingest.read_lscc(os.path.join(GOLDEN, f"x2dgl_{name}.lscc"))
    assert n == int(golden[f"{name}_n"]) and pairs.dtype == np.int32
    assert np.array_equal(pairs, golden[f"{name}_lines"][:, :2])


@pytest.mark.parametrize("name", NAMES)
def test_numpy_restatement_is_the_references_graph(golden, name):
    agrees(build_csr_numpy(golden[f"{name}_lines"][:, :2], int(golden[f"{name}_n"])), golden, name)


@pytest.mark.parametrize("name", NAMES)
def test_emulator_build_is_the_references_graph(golden, name):
    from tests.hipemu.emu_driver import emu_lib
    from tests.hipemu.emu_logreg import emu_ptr

    out = GraphBuildEngine(emu_lib(), emu_ptr, "cpu").build(golden[f"{name}_lines"][:, :2], int(golden[f"{name}_n"]))
    agrees({k: v.numpy() for k, v in out.items()}, golden, name)


def test_fixtures_cover_what_they_claim(golden):
    small = golden["small_lines"]
    assert (small[:, 0] == small[:, 1]).sum() == 3 and (small[:, 2] != 1).any()
    assert int(golden["small_log"][0]) == int(golden["tie_log"][0])
    assert int(np.diff(golden["hub_row_ptr"]).max()) > 64
