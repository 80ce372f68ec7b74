"""Device tier of tests/test_wide_edges_emu.py and of the small API-path cases of tests/test_wide_encoder_emu.py: the any-width
encoder and the dense head (csrc/ginx.hip) on a real MI355X at the edges the sampled batches of tests/test_wide_step_gpu.py and
tests/test_wide_encoder_gpu.py (widths 128 / 256, everything aligned) never reach, each against oracle/encoder.py in float64.

The cases, their inputs and their bars are the emulator tier's: one set of bodies, tests/wide_edges_check.py, run with the
gfx950 library on ``cuda`` tensors.  Inputs are generated on the CPU from the emulator tier's seeds and then moved, so both tiers
run the same numbers.  The emulator is lock-step, and its matrix-core, LDS and atomic operations are restatements: a missing
barrier, a cross-wave LDS reuse in the prefetch-ahead GEMM loops, a lane-layout slip that only a partial tile exposes, an
LDS-atomic or fp64-atomic path and a stale-row read past node_off[B] can only show here.  Every body also asserts that torch's
fp32 run of the oracle is inside the gradient bar against float64 (a bad input fails as such, not as a wrong kernel).

Batches: B = 24, at most 2,112 rows; nothing is sampled from a large graph and no eigensolver runs.

Measured on an MI355X (worst gradient entry against float64, in units of the tensor's largest entry: the kernels | torch's fp32 run
of the oracle on the same inputs; bar 1e-3):
    fused step 66 / 66 / 3           1.4e-5 | 2.7e-5         fused step 130 / 65 / 3          3.3e-6 | 1.2e-5
    API path 320 / 320 / 2           1.7e-4 | 2.2e-4         degree table 1023 x 16           2.5e-4 | 5.1e-4
    stale rows, 1023 live            1.3e-4 | 1.3e-4         stale rows, 1024 live            4.8e-4 | 4.8e-4
    stale rows, 1025 live            1.1e-4 | 1.1e-4         stale rows, 2049 live            4.5e-5 | 4.5e-5
    API path 96 / 80 / 3             4.1e-4 | 3.6e-4         API path 72 / 40 / 2             3.6e-4 | 7.3e-4
    head, d q: D 65 / 130 x K 4095 / 4096 / 4097 / 8192 <= 4.2e-7;  65 rows 2.8e-7;  one row 1.6e-7;  E2E D 65, B 40: 3.6e-7
All 21 cases passed on first contact with the device.  Wall time of the file: 5 s (the slowest case, the first, 2.0 s)."""
import pytest

from tests import wide_edges_check as C
from tests.wide_edges_check import GPU

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hidden,out", [(66, 66), (130, 65)])
def test_fused_step_at_widths_off_the_16_byte_grid_on_device(hidden, out):
    """widths that are no multiple of four: GEMM operands and BatchNorm parameters at offsets of the flat buffer that are not
    16-byte aligned (asserted on the device pointers), 3 layers, K = 96"""
    C.check_fused_step_off_grid(GPU, hidden, out)


def test_api_path_above_256_columns_on_device(monkeypatch):
    """hidden = out = 320: every 256-column loop (spmm, pooling, column sums, normalisation) takes a second, partial trip"""
    C.check_api_above_256(GPU, monkeypatch)


@pytest.mark.parametrize("n_live", [1023, 1024, 1025, 2049])
def test_fused_step_on_hand_built_batches_over_stale_rows_on_device(n_live):
    """node_cap 2,112; a 2,100-row batch goes first through the same workspaces, the dead input rows are NaN, the hub has degree
    530 (above max_degree); the checked step is the second"""
    C.check_stale_rows_step(GPU, n_live)


def test_degree_embedding_table_larger_than_lds_on_device(monkeypatch):
    """max_degree 1023 x 16 > kFeatMaxElems: the global-atomic kernel ginx_feat_bwd_atomic_kernel, with a 1,100-neighbour hub; forward
    and every parameter gradient (tests/wide_edges_check.py::check_degree_table says why this seed)"""
    C.check_degree_table(GPU, monkeypatch)


@pytest.mark.parametrize("D", [65, 130])
@pytest.mark.parametrize("K", [4095, 4096, 4097, 8192])
def test_wide_head_off_grid_widths_and_long_queues_on_device(D, K):
    """both sides of the split reduction of d loss / d q (fp64 atomics from K = 4096), two steps, a wrapping ring pointer, the
    queue after the enqueue exactly"""
    C.check_head(GPU, D, K)


@pytest.mark.parametrize("Bq", [65, 1])
def test_wide_head_second_row_tile_and_single_row_on_device(Bq):
    """D = 65, K = 200 with 65 rows (the second 64-row M-tile of the logits and d q products) and with one row"""
    C.check_head(GPU, 65, 200, Bq=Bq)


def test_wide_e2e_head_off_grid_width_on_device():
    """mode 1 (K = B, the grad_mem product) at D = 65 with B = 40"""
    C.check_e2e_head(GPU, 40, 65)


@pytest.mark.parametrize("hidden,out,layers", [(96, 80, 3), (72, 40, 2)])
def test_api_path_at_small_widths_on_device(hidden, out, layers, monkeypatch):
    """training forward and backward, running statistics, save / load, eval mode, embed_views; d_in = 49 and the widths
    72 / 96 / 40 / 80 leave partial k-tiles and edge tiles"""
    C.check_api_path(GPU, hidden, out, layers, monkeypatch)
