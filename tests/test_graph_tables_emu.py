"""gcc_graph_tables / gcc_graph_tables_hub_adj (gcc_amd/csrc/graph_tables.hip) on the lock-step emulator against the host's tables:
the checks of tests/graph_tables_check.py.  (The emulator runs workgroups one after another: it sees the kernels' logic at every
tile boundary, not a race between workgroups -- tests/test_graph_tables_gpu.py repeats the calls and changes the grid for that.)"""
import re

import pytest

from tests import graph_tables_check as C
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_logreg import emu_ptr


@pytest.fixture(scope="module")
def gt():
    return C.Gt(emu_lib(), emu_ptr, "cpu")


@pytest.mark.parametrize("name", C.NAMES)
def test_tables_are_the_hosts(gt, name):
    C.check_case(gt, name)


@pytest.mark.parametrize("name", [f"n{C.T + 1}", "three_shards"])
def test_grid_size_does_not_change_a_bit(gt, name):
    C.check_case(gt, name, grids=(0, 1, 3))


def test_known_values(gt):
    C.check_known_values(gt)


def test_no_table_above_the_byte_limit_or_when_not_asked_for(gt):
    C.check_hub_table_limits(gt)


@pytest.mark.parametrize("name", ["powerlaw", "powerlaw_three_shards"])
def test_oracle_draws_the_same_seeds_from_both_cdfs(gt, name):
    C.check_seeds(gt, name)


def test_shard_without_weight_sets_the_bit_and_never_a_nan(gt):
    C.check_empty_shard(gt)


def test_sizes_short_workspace_bad_shards_and_null_members_are_refused_by_name(gt):
    C.check_refusals(gt)


def test_product_path_refuses_cpu_tensors():
    C.check_cpu_tensor_refused(emu_lib())


def test_exported_tiles_are_the_headers():
    from gcc_amd import _cabi

    src = open(_cabi.HEADER_PATH).read()
    for name in ("GRAPH_TABLES_SCAN_TILE", "GRAPH_TABLES_ENTRY_TILE", "GRAPH_TABLES_HUB_DEGREE", "GRAPH_TABLES_SUMMARY_WORDS",
                 "STATUS_GRAPH_TABLES_EMPTY_SHARD"):
        assert int(re.search(rf"#define GCC_{name} (\d+)", src).group(1)) == getattr(_cabi, name), name
    from gcc_amd.graph import HUB_TABLE_DEGREE

    assert HUB_TABLE_DEGREE == _cabi.GRAPH_TABLES_HUB_DEGREE
