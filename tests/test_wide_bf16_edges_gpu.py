"""Device tier of the small cases of tests/test_wide_bf16_emu.py: ``--encoder-dtype bf16`` / ``--nce-dtype bf16`` above 64
channels (ginx_gemm_bf16_kernel on v_mfma_f32_16x16x32_bf16, gcc_ncex_forward_dt) on a real MI355X at partial k-tiles, edge
tiles, stale rows and off-grid head shapes, each against tests/bf16_reference.py -- the rule in float64 on the rounded values --
under the ``Bars`` rule: a bar is its f32-mode value or twice the rounded oracle's fp32-vs-float64 gap, whichever is larger, and
that gap is measured on the reference, never on the code under test.

The cases, inputs and bars are the emulator tier's (one set of bodies: tests/wide_edges_check.py; inputs generated on the CPU
from the same seeds, then moved).  What this file adds to tests/test_wide_bf16_gpu.py is RESOLUTION: at hidden 256 and 5 layers
the rule's own gap widens the gradient bar to ~8e-2 of a tensor's largest entry; at 2 and 3 layers the gaps are 1e-7 to a few
1e-3, so a lane-layout slip in a partial tile or a missing barrier shows.  For every kind of quantity whose gap is below 1e-3 the
shared bodies assert that no bar was widened beyond what that gap allows (``assert_resolution`` prints error | gap per kind),
and the tests below assert that the kinds named there do have such a gap.

Batches: B = 24, at most 2,112 rows; nothing is sampled from a large graph and no eigensolver runs.

Measured on an MI355X (err = the kernels, gap = the rounded oracle's fp32 run, both against its float64 run, in the unit of each
bar; gradients in units of the tensor's largest entry):
    case                   features err | gap     pooled err | gap       gradients err | gap     running statistics err | gap
    API 96 / 80 / 3        1.6e-7 | 1.5e-7        8.5e-6 | 3.5e-5        8.2e-4 | 1.2e-3         5.1e-7 | 5.1e-7
    API 72 / 40 / 2        1.1e-7 | 2.9e-7        5.4e-6 | 4.9e-5        4.2e-4 | 1.1e-3         6.0e-8 | 6.9e-8
    stale rows, 1023 live  1.4e-7 | 1.5e-6        2.7e-5 | 2.5e-4        6.1e-4 | 2.3e-3         1.9e-6 | 7.6e-6
    stale rows, 1025 live  1.3e-7 | 1.4e-6        3.7e-5 | 1.7e-4        7.2e-4 | 5.0e-3         1.7e-6 | 8.7e-6
    stale rows, 2049 live  5.1e-6 | 5.1e-6        2.3e-3 | 2.2e-3        9.2e-4 | 2.4e-3         3.6e-7 | 1.3e-6
    fused step 128 / 2: embeddings 7.2e-6 | 1.2e-7, loss / prob / gradient norm 8.9e-7 | 2.1e-7, gradients 2.3e-4 | 1.9e-4,
        running statistics 6.0e-8 | 7.5e-8, model_ema 5.9e-6 | 7.9e-7
    head (D, K, rows), worst of three steps: logits <= 9.5e-7 | 1.2e-6; d q (80, 200, 40) 4.8e-7 | 1.2e-7, (96, 4400, 40)
        8.1e-6 | 2.0e-6, (80, 200, 65) 5.4e-5 | 1.2e-7, (80, 200, 1) 5.3e-8 | 5.4e-8; E2E gradients (128, B 48) 1.7e-7 | 2.4e-7,
        (65, B 40) 1.2e-7 | 1.9e-7
So the gradient bars here are 1e-3 to 1e-2 of a tensor's largest entry (8e-2 at 256 / 5 layers), every other bar is its f32-mode
value, and the errors sit at or below the reference's own gap.  Wall time of the file: 3 s (6 s together with
tests/test_wide_edges_gpu.py).

ONE CASE FAILED ON FIRST CONTACT, and the kernels were changed for it: test_the_flag_does_something_and_f32_mode_is_untouched_on_device.
"f32 mode is bit-identical to a model built without the keyword" did not hold for two of the 30 tensors, keyword or not: two runs
of the SAME f32 model differed in d degree_embedding.weight (31 to 68 of 8,208 entries, up to 2.7e-7 of its largest entry: the fp32
LDS and global atomics of ginx_feat_bwd_kernel added in the order the waves arrived) and in d gnn.ginlayers.0.apply_func.bn.weight
(1 of 96 entries, 7.6e-9: the fp64 atomics of ginx_colsum_kernel, rounded to fp32 after a sum that cancels).  Both reductions now
add per-block partial sums in a fixed order (ginx_colsum_reduce_kernel, ginx_feat_reduce_kernel): all 30 tensors were bit-identical
in nine runs of three models, and the step at hidden 256 takes the time it took (2.79 ms, alternated runs against the parent's
library)."""
import pytest

from tests import wide_edges_check as C
from tests.wide_edges_check import GPU

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hidden,out,layers", [(96, 80, 3), (72, 40, 2)])
def test_bf16_api_path_vs_rounded_oracle_on_device(hidden, out, layers, monkeypatch):
    """features, pooled outputs, every parameter gradient, running statistics, eval mode and embed_views; d_in = 49 and the
    widths 72 / 96 / 40 / 80 leave partial k-tiles and edge tiles that are zero-filled in LDS"""
    bars = C.check_bf16_api_path(GPU, hidden, out, layers, monkeypatch)
    assert bars.gap("features") < 1e-3 and bars.gap("running statistics") < 1e-3     # (these kinds do have the resolution)


@pytest.mark.parametrize("n_live", [1023, 1025, 2049])
def test_bf16_on_hand_built_batches_over_stale_rows_on_device(n_live, monkeypatch):
    """72 / 72 / 2 in node_cap 2,112 after a 2,100-row batch: the bf16 staging must never read the stale or NaN rows; two and
    three 1,024-row split-K slabs of the weight gradients, the last one a single row"""
    C.check_bf16_stale_rows(GPU, n_live, monkeypatch)


@pytest.mark.parametrize("D,K,Bq", [(80, 200, 40), (96, 4400, 40), (80, 200, 65), (80, 200, 1)])
def test_bf16_wide_moco_head_vs_rounded_reference_on_device(D, K, Bq):
    """three steps with a wrapping ring pointer, the queue after the enqueue exactly; K >= 4096: the split reduction of
    d loss / d q; 65 rows: the second 64-row M-tile; one row"""
    bars = C.check_bf16_head(GPU, D, K, Bq=Bq)
    assert bars.gap("d q") < 1e-3 and bars.gap("logits") < 1e-3


@pytest.mark.parametrize("Bq,D", [(48, 128), (40, 65)])
def test_bf16_wide_e2e_head_vs_rounded_reference_on_device(Bq, D):
    """mode 1 (K = B, the grad_mem product)"""
    bars = C.check_bf16_e2e_head(GPU, Bq, D)
    assert bars.gap("gradients") < 1e-3 and bars.gap("logits") < 1e-3


def test_fused_wide_step_bf16_on_fixed_views_on_device():
    """the fused step at 128 / 2 layers with both dtypes bf16: every kind of bf16 product, the rule's gap near the f32 bars"""
    bars = C.check_bf16_fused_step(GPU)
    assert bars.gap("gradients") < 1e-3 and bars.gap("embeddings") < 1e-3


def test_the_flag_does_something_and_f32_mode_is_untouched_on_device(monkeypatch):
    """bf16 differs from f32 on the same inputs; f32 mode is bit-identical to a model built without the keyword.

    (failed on first contact with the device, on two tensors summed with atomics: module docstring)"""
    C.check_bf16_flag(GPU, monkeypatch)


def test_f32_products_are_bit_identical_between_two_models_on_device(monkeypatch):
    """the part of the flag check that held before the atomic reductions were given a fixed order: features, pooled outputs, running
    statistics and every Linear weight gradient of a model built without the keyword and of one built with encoder_dtype="f32" """
    C.check_f32_products_are_reproducible(GPU, monkeypatch)
