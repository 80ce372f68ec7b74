"""gcc_graph_build / gcc_graph_check (gcc_amd/csrc/graph_build.hip) on a real MI355X: the checks of tests/graph_build_check.py on
every case, each call repeated (the rows fill in whatever order the atomics arrive: only the device can show a race between
workgroups), ``DeviceGraph(validate="device")``, and a built graph under the sampler."""
import numpy as np
import pytest

from tests import graph_build_check as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gb():
    from gcc_amd import _cabi

    return C.Gb(_cabi.load(), _cabi.dev_ptr, "cuda:0")


@pytest.mark.parametrize("name", C.NAMES)
def test_build_is_the_restatements(gb, name):
    C.check_parity(gb, name)


@pytest.mark.parametrize("name", ["powerlaw", f"star{2 * C.L + 3}x3", f"star{2 * C.L + 3}straddle", f"star{C.L}x3", f"star{C.W + 1}x3",
                                  "one_edge_ten_times", f"n{C.T + 1}"])
def test_two_calls_and_any_order_of_the_lines_give_the_same_bits(gb, name):
    C.check_order_independence(gb, name, calls=2)


def test_ids_outside_the_range_set_the_bit_and_the_rest_builds(gb):
    C.check_bad_ids(gb)


def test_sizes_short_workspace_and_null_members_are_refused_by_name(gb):
    C.check_refusals(gb)


def test_cpu_tensor_is_refused(gb):
    C.check_cpu_tensor_refused(gb.lib)


@pytest.mark.parametrize("name", sorted(C.violations()))
def test_one_violation_sets_exactly_its_bit_and_check_contracts_message(gb, name):
    C.check_violation(gb, name)


def test_multigraph_mode_compares_copy_counts(gb):
    C.check_multigraph_mode(gb)


@pytest.fixture(scope="module")
def parent():
    from gcc_amd.graphgen import powerlaw_graph

    return powerlaw_graph(2000, 12000)


def test_device_graph_validates_on_the_device(parent):
    from gcc_amd.graph import DeviceGraph

    rp, ci = parent
    g = DeviceGraph(rp, ci, rw_hops=16, device="cuda:0", validate="device")
    assert g.contract_checked and g.c.flags & 1
    host = DeviceGraph(rp, ci, rw_hops=16, device="cuda:0", validate=True)
    assert g.num_hubs == host.num_hubs and g.max_degree == host.max_degree
    with pytest.raises(ValueError, match="validate 'gpu'"):
        DeviceGraph(rp, ci, rw_hops=16, device="cuda:0", validate="gpu")


def test_device_graph_raises_check_contracts_message(parent):
    from gcc_amd.graph import DeviceGraph
    from gcc_amd.graphgen import check_contract

    rp, ci = parent
    row = int(np.argmax(np.diff(rp)))
    short = rp.copy()
    short[row + 1:] -= 1
    lop = np.delete(ci, int(rp[row]))
    with pytest.raises(ValueError) as host:
        check_contract(short, lop)
    with pytest.raises(ValueError) as dev:
        DeviceGraph(short, lop, rw_hops=16, device="cuda:0", validate="device")
    assert str(dev.value) == str(host.value) and "not symmetric" in str(dev.value)


def test_built_graph_samples_like_the_same_csr_from_the_host(gb):
    """lines -> the engine's CSR -> DeviceGraph -> one batch, against the restatement's CSR through the host-checked path"""
    from gcc_amd.graph import DeviceGraph
    from gcc_amd.sampler import DeviceRWRSampler

    n, lines = C.CASES["powerlaw"]
    out = gb.engine.build(lines, n)
    gb.engine.check_status(out)
    ref = C.reference("powerlaw")
    batches = []
    for rp, ci, validate in ((out["row_ptr"].cpu().numpy(), out["col_idx"].cpu().numpy(), "device"), (ref["row_ptr"].copy(), ref["col_idx"].copy(), True)):
        g = DeviceGraph(rp, ci, rw_hops=16, device="cuda:0", validate=validate)
        s = DeviceRWRSampler(g, batch_size=8, run_seed=5)
        q, k = s.sample(0)
        s.check_status()
        batches.append((q.csr_numpy(), k.csr_numpy()))
    for a, b in zip(*batches):
        assert a["parent_nid"].size > 8
        for key in a:
            assert np.array_equal(a[key], b[key]), key
