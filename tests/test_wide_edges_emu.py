"""The any-width encoder (csrc/ginx.hip) and the wide head at the edges the sampled batches of the other tests never reach, each
against oracle/encoder.py run in float64.  Emulator tier; the device tier is tests/test_wide_edges_gpu.py (the same cases through the same bodies: tests/wide_edges_check.py).

- widths that are not multiples of four through the fused step (MoCoTrainStep._body on the any-width engines): parameters at offsets of the flat
  buffer that are not 16-byte aligned, so the GEMM's, BatchNorm's, pooling's and spmm's scalar paths run on them;
- a width above 256 through the API path: the 256-column loops of spmm, pooling and the column sums take a second trip;
- hand-built batches of 1023, 1024, 1025 and 2049 live rows (the weight gradients' 1,024-row slabs and the end of the last one)
  inside a larger node capacity whose rows past the live count hold a larger earlier batch's activations and gradients, with
  NaN in the dead input rows, empty and one-node subgraphs, isolated nodes and a node whose degree exceeds max_degree;
- a degree-embedding table too large for LDS (the global-atomic kernel ginx_feat_bwd_atomic_kernel);
- the wide head at D = 65, 130 on both sides of its long-reduction split (K = 4095 / 4096), with 65 rows (a second 64-row M-tile
  of the logits and d q products) and with one row, and its E2E mode (K = B, the grad_mem product) at D = 65."""
import pytest

from tests import wide_edges_check as C
from tests.wide_edges_check import B, EMU, encoder, hand_batch  # noqa: F401  (names other test files import from here)
from tests.wide_edges_check import ScriptedSampler as _ScriptedSampler  # noqa: F401
from tests.wide_edges_check import fused_step as _fused_step  # noqa: F401
from tests.wide_edges_check import masks as _masks  # noqa: F401


@pytest.mark.parametrize("hidden,out", [(66, 66), (130, 65)])
def test_fused_step_at_widths_off_the_16_byte_grid(hidden, out):
    C.check_fused_step_off_grid(EMU, hidden, out)


def test_api_path_above_256_columns(monkeypatch):
    """hidden = out = 320: every 256-column loop (spmm, pooling, column sums, normalisation) takes a second, partial trip"""
    C.check_api_above_256(EMU, monkeypatch)


@pytest.mark.parametrize("n_live", [1023, 1024, 1025, 2049])
def test_fused_step_on_hand_built_batches_over_stale_rows(n_live):
    """node_cap 2,112 for every case; the first step runs a 2,100-row batch through the same workspaces (forward, backward), so the
    rows between the live count and the capacity hold its activations and gradients; the checked step is the second"""
    C.check_stale_rows_step(EMU, n_live)


def test_degree_embedding_table_larger_than_lds(monkeypatch):
    """max_degree 1023 x 16 columns = 16,384 floats > the 10,240 of ginx_feat_bwd_kernel's LDS copy: the scatter-add goes straight
    to global memory.  A 1,100-neighbour hub is clamped to row 1,023.  (Such a hub is an outlier every BatchNorm of the layer sees:
    on some seeds of this batch one pre-activation sits within fp32 rounding of a ReLU kink, and then the kernels and torch's fp32
    run are off from float64 by the same 1e-3 of a tensor's scale.  This seed keeps torch's fp32 run inside the bar too.)"""
    C.check_degree_table(EMU, monkeypatch)


@pytest.mark.parametrize("D", [65, 130])
@pytest.mark.parametrize("K", [4095, 4096, 4097, 8192])
def test_wide_head_off_grid_widths_and_long_queues(D, K):
    """MemoryMoCo(D, K) on the dense head: logits, loss, prob, d loss / d q against float64 (K >= 4096: the reduction over the
    queue is split over workgroups with fp64 atomics; 4095 is the last K that is not), the queue after the enqueue, over two steps"""
    C.check_head(EMU, D, K)


@pytest.mark.parametrize("Bq", [65, 1])
def test_wide_head_second_row_tile_and_single_row(Bq):
    """every other head test has 40 rows: 65 enter the second 64-row M-tile of the logits and d q products, 1 leaves the first
    nearly empty (D = 65, K = 200)"""
    C.check_head(EMU, 65, 200, Bq=Bq)


def test_wide_e2e_head_off_grid_width():
    """mode 1 (K = B, the grad_mem product) at D = 65 with B = 40; the other E2E head tests use D = 128"""
    C.check_e2e_head(EMU, 40, 65)
