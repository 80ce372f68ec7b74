"""gcc_graph_build / gcc_graph_check (gcc_amd/csrc/graph_build.hip) on the lock-step emulator against the NumPy restatement of the
converter's rule: the checks of tests/graph_build_check.py.  (The emulator runs workgroups one after another: it sees the kernels'
logic at every class boundary, not a race between workgroups -- tests/test_graph_build_gpu.py repeats the calls for that.)"""
import pytest

from tests import graph_build_check as C
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_logreg import emu_ptr


@pytest.fixture(scope="module")
def gb():
    return C.Gb(emu_lib(), emu_ptr, "cpu")


@pytest.mark.parametrize("name", C.NAMES)
def test_build_is_the_restatements(gb, name):
    C.check_parity(gb, name)


@pytest.mark.parametrize("name", ["powerlaw", f"star{2 * C.L + 3}x3", f"star{C.L}straddle", "one_edge_ten_times"])
def test_any_order_of_the_lines_gives_the_same_bits(gb, name):
    C.check_order_independence(gb, name)


def test_ids_outside_the_range_set_the_bit_and_the_rest_builds(gb):
    C.check_bad_ids(gb)


def test_sizes_short_workspace_and_null_members_are_refused_by_name(gb):
    C.check_refusals(gb)


def test_product_path_refuses_cpu_tensors():
    C.check_cpu_tensor_refused(emu_lib())


@pytest.mark.parametrize("name", sorted(C.violations()))
def test_one_violation_sets_exactly_its_bit_and_check_contracts_message(gb, name):
    C.check_violation(gb, name)


def test_multigraph_mode_compares_copy_counts(gb):
    C.check_multigraph_mode(gb)


def test_exported_class_boundaries_are_the_headers():
    import re

    from gcc_amd import _cabi

    src = open(_cabi.HEADER_PATH).read()
    for name in ("GRAPH_BUILD_WAVE_ROW", "GRAPH_BUILD_LDS_ROW", "GRAPH_BUILD_SCAN_TILE", "STATUS_GRAPH_BUILD_BAD_ID",
                 "STATUS_GRAPH_CHECK_SPAN", "STATUS_GRAPH_CHECK_ZERO_DEGREE", "STATUS_GRAPH_CHECK_RANGE", "STATUS_GRAPH_CHECK_UNSORTED",
                 "STATUS_GRAPH_CHECK_SELF_LOOP", "STATUS_GRAPH_CHECK_DUPLICATE", "STATUS_GRAPH_CHECK_ASYMMETRIC"):
        assert int(re.search(rf"#define GCC_{name} (\d+)", src).group(1)) == getattr(_cabi, name), name
