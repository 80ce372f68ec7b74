"""Device tier of tests/test_gin_edges_emu.py: the fused 64-channel GIN pass (csrc/encoder.hip, encoder_bwd.hip) on a real MI355X
at its shape edges, one training-mode forward and backward per case against oracle/encoder.py in float64.  One body,
tests/gin_edges_check.py::check_case, run with the gfx950 library on ``cuda`` tensors; inputs and models come from the emulator
tier's seeds, so both tiers run the same numbers.  Every batch has at most 200 nodes.

Measured on an MI355X (feat: worst absolute error; gradients: worst entry in units of the tensor's largest entry, bar 1e-3; each
the kernels | torch's fp32 run of the oracle, against float64):
    case                             feat               gradients
    one_graph_20                     1.5e-7 | 1.1e-7    1.1e-5 | 1.2e-5
    one_graph_64                     7.1e-8 | 8.1e-8    5.9e-6 | 3.6e-6
    one_graph_65                     8.3e-8 | 8.0e-8    8.3e-6 | 1.6e-5
    cap_equals_n_128                 1.2e-7 | 8.6e-8    4.6e-6 | 4.9e-6
    cap_equals_n_73                  1.5e-7 | 2.0e-7    1.0e-5 | 7.0e-6
    rows_hint_1                      1.7e-7 | 2.3e-7    7.3e-6 | 7.0e-6
    readout_b15                      9.3e-7 | 5.3e-7    1.4e-5 | 1.9e-5
    readout_b16                      6.6e-7 | 6.8e-7    1.8e-5 | 5.0e-5
    readout_b17                      5.6e-7 | 4.0e-7    3.0e-5 | 2.2e-5
    readout_b33                      6.0e-7 | 5.5e-7    4.0e-5 | 3.2e-5
    empty_and_single_graphs          3.1e-7 | 2.0e-7    6.6e-6 | 9.5e-6
    stripped_rows_at_tile_borders    8.8e-7 | 5.8e-7    2.3e-5 | 3.3e-5
    hub_max_degree_4                 3.0e-7 | 1.1e-6    6.6e-6 | 4.2e-5
    hub_max_degree_2                 3.5e-7 | 2.2e-6    2.7e-5 | 1.5e-4
    hub_table_10240_floats           1.7e-7 | 7.7e-7    1.2e-5 | 1.4e-5
    layers_2                         7.2e-8 | 9.6e-8    4.2e-6 | 2.4e-6
    layers_3                         1.1e-7 | 1.2e-7    3.1e-6 | 2.4e-6
    layers_9                         4.5e-7 | 6.5e-7    1.4e-5 | 1.6e-5
    cols_32_31                       2.0e-7 | 1.2e-7    5.2e-6 | 3.4e-6
    cols_30_17                       2.5e-7 | 1.3e-7    3.6e-6 | 2.6e-6
    cols_32_5                        2.1e-7 | 2.1e-7    5.8e-6 | 1.1e-5
    cols_6_16                        2.1e-7 | 1.2e-7    5.9e-6 | 2.7e-6
    cols_2_1                         2.3e-7 | 1.8e-7    1.6e-5 | 7.0e-6
    seed_local                       1.1e-7 | 1.5e-7    3.8e-6 | 4.8e-6
    accumulate                       2.6e-7 | 1.5e-7    4.9e-6 | 4.5e-6
All 25 cases passed on first contact with the device.  Wall time of the file: 5 s (the first case, which loads the library, 1.1 s;
every other one below 0.2 s)."""
import pytest

from tests import gin_edges_check as G
from tests.wide_edges_check import GPU

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(G.CASES))
def test_gin_pass_edge_case_vs_float64_oracle_on_device(name):
    G.check_case(GPU, name)
