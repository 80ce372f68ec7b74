"""``--encoder-dtype bf16`` / ``--nce-dtype bf16`` above 64 channels: the any-width encoder and the dense head of
gcc_amd/csrc/ginx.hip with bf16 operands on v_mfma_f32_16x16x32_bf16 (ginx_gemm_bf16_kernel; gcc_ginx_pass.gemm_dtype = 1,
gcc_ncex_forward_dt) against tests/bf16_reference.py -- the rule restated with plain torch and run in float64 on the rounded
values.  Emulator tier; the device tier is tests/test_wide_bf16_edges_gpu.py (the same small cases through the same bodies,
tests/wide_edges_check.py) and tests/test_wide_bf16_gpu.py (hidden 256 on a sampled batch).

Bars: those tests/test_wide_encoder_emu.py uses for the f32 mode -- features rtol 2e-4 / atol 2e-5 (pooled outputs atol 2e-4,
running statistics rtol 1e-4 / atol 1e-5), gradients 1e-3 of the tensor's largest entry against float64.  One thing is new in
this mode: an activation that differs by one fp32 ulp between two implementations can sit on a bf16 rounding boundary, and then
the two round it 2^-8 of its size apart.  That is a property of the rule, not of an implementation of it, so where it needs room
the room is MEASURED, never chosen: the same rounded oracle is run in fp32 and in float64 (two implementations of the rule,
neither the code under test) and a bar becomes max(its f32-mode value, twice that gap) -- :class:`Bars`.

The gap is taken per KIND of quantity, in the unit its bar is stated in: one figure for the features, one for the pooled outputs,
one for the running statistics, and for the gradients the worst entry of any tensor in units of that tensor's largest entry.
Which activations tip is decided by the last bit of an fp32 sum, and one tip moves everything downstream of it by an amount that
depends on where it happened to fall (measured at 256 / 256 / 5: torch's fp32 run and the kernels each tip 4 of the 144,128
activations behind the first BatchNorm -- different ones; torch's move the next pooled output by 9.9e-4, the kernels' by 3.6e-3;
two layers on both have tipped ~15 % of all activations).  The gap of ONE tensor is a single draw of that lottery; the worst over
the tensors of a kind is what the rule needs.  Every comparison prints its figures before it is asserted.

Measured here (emulator; err = this code, gap = the rounded oracle's fp32 run, both against its float64 run; gradients in units
of the tensor's largest entry):
    widths / layers   features err | gap      pooled err | gap        gradients err | gap     running statistics err | gap
    128 / 128 / 5     1.3e-4 | 6.3e-4         4.8e-2 | 2.0e-1         3.0e-2 | 1.3e-1         2.9e-4 | 3.2e-3
    96 / 80 / 3       1.6e-7 | 3.2e-7         1.0e-5 | 5.2e-5         8.2e-4 | 1.3e-3         5.1e-7 | 5.1e-7
    256 / 256 / 5     3.8e-4 | 3.2e-4         4.2e-1 | 4.5e-1         7.1e-2 | 6.8e-2         3.5e-3 | 3.1e-3
    72 / 40 / 2       2.9e-7 | 2.8e-7         4.9e-5 | 4.8e-5         3.0e-4 | 1.5e-3         6.0e-8 | 6.9e-8
    fused step, 128 / 2 layers: embeddings 7.2e-6 | 6.9e-7, gradients 2.3e-4 | 1.9e-4 (inside the f32 bars)
    head (D, K) = (128, 96), (80, 200), (96, 4400), E2E: logits <= 1.5e-6 | 1.5e-6, d q <= 3.8e-6 | 5.0e-7 of its largest entry
    head (80, 200) with 65 rows / one row, E2E at D = 65: logits <= 8.1e-7 | 8.1e-7, d q <= 5.4e-5 | 2.4e-7, gradients 1.9e-7 | 1.9e-7
Up to three layers the kernels follow the rule to fp32 rounding; at five the rule itself is conditioned as the gap column says.
"""
import ctypes

import pytest
import torch

from gcc_amd import _cabi
from gcc_amd.contrast import MemoryMoCo
from gcc_amd.encoder import GraphEncoder
from tests import wide_edges_check as C
from tests.test_wide_edges_emu import _masks, hand_batch  # noqa: F401
from tests.test_wide_encoder_emu import emu_wide_engine, fixed_views
from tests.wide_edges_check import EMU, check_bf16_against_rounded_oracle  # noqa: F401


def wide_encoder(hidden, out, layers=5, **kw):
    return GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=512,
                        freq_embedding_size=16, degree_embedding_size=16, output_dim=out, node_hidden_dim=hidden,
                        edge_hidden_dim=hidden, num_layers=layers, num_step_set2set=6, num_layer_set2set=3, norm=True,
                        gnn_model="gin", degree_input=True, **kw)


def emu_wide_nce(dtype="bf16"):
    return EMU.wide_nce(dtype)


@pytest.mark.parametrize("hidden,out,layers", [(128, 128, 5), (96, 80, 3), (256, 256, 5), (72, 40, 2)])
def test_bf16_api_path_forward_backward_vs_rounded_oracle(hidden, out, layers, monkeypatch):
    """Forward features and pooled outputs, every parameter gradient, running statistics and eval mode against the rounded
    float64 oracle; d_in = 49 and the widths 72 / 96 / 40 / 80 leave partial k-tiles and edge tiles that are zero-filled in LDS."""
    C.check_bf16_api_path(EMU, hidden, out, layers, monkeypatch)


def test_the_flag_does_something_and_f32_mode_is_untouched(monkeypatch):
    """bf16 and f32 mode differ on the same inputs; f32 mode is bit-identical to a model built without the keyword"""
    C.check_bf16_flag(EMU, monkeypatch)


def test_f32_products_are_bit_identical_between_two_models(monkeypatch):
    """the products of the flag check (tests/test_wide_bf16_edges_gpu.py says what failed on hardware first): features, pooled
    outputs, running statistics and every Linear weight gradient"""
    C.check_f32_products_are_reproducible(EMU, monkeypatch)


@pytest.mark.parametrize("n_live", [1023, 1025, 2049])
def test_bf16_on_hand_built_batches_over_stale_rows(n_live, monkeypatch):
    """node_cap 2,112; a 2,100-row batch goes through the same workspace slots first (forward and backward), so the rows past the
    live count hold its activations and gradients, and the dead input rows are NaN: the bf16 staging must never read them.  1,025
    and 2,049 live rows span two and three 1,024-row split-K slabs of the weight gradients (the last one a single row)."""
    C.check_bf16_stale_rows(EMU, n_live, monkeypatch)


@pytest.mark.parametrize("D,K", [(128, 96), (80, 200), (96, 4400)])    # (K >= 4096: the split reduction of d loss / d q)
def test_bf16_wide_moco_head_vs_rounded_reference(D, K):
    """MemoryMoCo(inputSize > 64, nce_dtype="bf16"): dense logits, loss, prob and d loss / d q against the queue BEFORE the
    enqueue, under the rule in float64; the queue after the enqueue exactly; three steps with a wrapping ring pointer."""
    C.check_bf16_head(EMU, D, K)


@pytest.mark.parametrize("Bq", [65, 1])
def test_bf16_wide_head_second_row_tile_and_single_row(Bq):
    """65 rows enter the second 64-row M-tile of the logits and d q products, 1 leaves the first nearly empty (D = 80, K = 200)"""
    C.check_bf16_head(EMU, 80, 200, Bq=Bq)


def test_bf16_wide_head_differs_from_f32_head():
    torch.manual_seed(1)
    q = torch.nn.functional.normalize(torch.randn(40, 128), dim=1)
    k = torch.nn.functional.normalize(torch.randn(40, 128), dim=1)
    mem = torch.nn.functional.normalize(torch.randn(96, 128), dim=1)
    a = emu_wide_nce("f32").forward(q, k, mem, 0.07, 0)
    b = emu_wide_nce("bf16").forward(q, k, mem, 0.07, 0)
    assert torch.equal(a["out"][:, 0], b["out"][:, 0])                          # the positive logit stays f32
    assert not torch.equal(a["out"], b["out"]) and not torch.equal(a["grad_rows"], b["grad_rows"])


def test_bf16_wide_e2e_head_vs_rounded_reference():
    C.check_bf16_e2e_head(EMU, 48, 128)


def test_bf16_wide_e2e_head_off_grid_width():
    """mode 1 (K = B, the grad_mem product) at D = 65 with B = 40"""
    C.check_bf16_e2e_head(EMU, 40, 65)


def test_fused_wide_step_bf16_encoder_and_head_vs_rounded_oracle():
    """MoCoTrainStep._body at hidden 128 with --encoder-dtype bf16 and --nce-dtype bf16, one step.  One GIN layer (num_layers
    2): every kind of bf16 product runs -- z1 with k = 49, z2, d a1, d agg, dW1 and dW0 over the node dimension, the head's three --
    while the rule's own fp32-vs-float64 gap stays near the f32 bars, so the comparison keeps its resolution (each further layer
    multiplies that gap: see the module docstring)."""
    C.check_bf16_fused_step(EMU)


def test_refusals():
    with pytest.raises(NotImplementedError, match="compute in f32"):
        wide_encoder(64, 64, 5, encoder_dtype="bf16")
    with pytest.raises(NotImplementedError, match="compute in f32"):
        GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=512, freq_embedding_size=16,
                     degree_embedding_size=16, output_dim=64, node_hidden_dim=64, edge_hidden_dim=64, num_layers=2, norm=True,
                     gnn_model="gat", degree_input=True, encoder_dtype="bf16")
    with pytest.raises(ValueError, match="encoder_dtype"):
        wide_encoder(128, 128, 5, encoder_dtype="fp8")
    # the C ABI refuses gemm_dtype = 2, in the encoder pass and in the head
    model = wide_encoder(72, 40, 2)
    eng = emu_wide_engine()
    q, _ = fixed_views()
    p, _buf = eng.make_pass(model, q, training=True)
    p.gemm_dtype = 2
    with pytest.raises(RuntimeError, match="gemm_dtype 2"):
        eng.forward(p)
    grads = _cabi.GccGinGrads()
    assert eng.lib.gcc_ginx_backward(ctypes.byref(p), 1, ctypes.byref(grads), None) != 0
    assert b"gemm_dtype 2" in eng.lib.gcc_last_error()
    nce = emu_wide_nce()
    o = dict(t=torch.zeros(8, 200))
    ptr = o["t"].data_ptr()
    rc = nce.lib.gcc_ncex_forward_dt(ptr, ptr, ptr, 2, 4, 72, 1.0, 0, ptr, ptr, ptr, None, ptr, ptr, ptr, 2, None)
    assert rc != 0 and b"gemm_dtype 2" in nce.lib.gcc_last_error()
    with pytest.raises(ValueError, match="nce_dtype"):
        MemoryMoCo(128, None, 96, 0.07, use_softmax=True, nce_dtype="fp8")
