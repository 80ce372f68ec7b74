"""The fused 64-channel GIN pass (csrc/encoder.hip, encoder_bwd.hip) at its shape edges on the emulator build: one training-mode
forward and backward per case against oracle/encoder.py in float64.  The cases, inputs and bars are tests/gin_edges_check.py's;
the device tier is tests/test_gin_edges_gpu.py.  Also the two refusals of this path that used not to name their cause."""
import pytest
import torch

from tests import gin_edges_check as G
from tests.wide_edges_check import EMU


@pytest.mark.parametrize("name", list(G.CASES))
def test_gin_pass_edge_case_vs_float64_oracle(name):
    G.check_case(EMU, name)


def _encoder(**kw):
    from gcc_amd.encoder import GraphEncoder

    args = dict(positional_embedding_size=32, max_degree=512, degree_embedding_size=16, output_dim=64, node_hidden_dim=64,
                num_layers=5, norm=True, gnn_model="gin", degree_input=True)
    args.update(kw)
    return GraphEncoder(**args)


def test_one_layer_model_is_refused_by_name():
    """num_layers = 1 leaves no GIN layer: a ValueError that names num_layers, from the constructor and from fill_weights"""
    from gcc_amd.encoder import fill_weights

    with pytest.raises(ValueError, match="num_layers=1"):
        _encoder(num_layers=1)
    model = _encoder(num_layers=2)
    del model.gnn.ginlayers[0]
    with pytest.raises(ValueError, match="num_layers"):
        fill_weights(model, lambda t: 0 if t is None else t.data_ptr())


def test_degree_table_above_lds_is_refused_by_name_in_backward_only():
    """(max_degree + 1) * degree_embedding_size above 10,240 floats: the forward-only training pass of a key encoder is served,
    gcc_gin_backward refuses and says why"""
    c = dict(G.CASES["cap_equals_n_73"], max_degree=512, emb=31)
    assert (c["max_degree"] + 1) * c["emb"] > G.EMB_LDS_FLOATS and c["pos"] + c["emb"] + 1 <= 64
    g, args, _ = G.build_batch(EMU, c)
    model, o32, _ = G.build_models(EMU, c)
    eng = EMU.gin_engine()
    p, buf = eng.make_pass(model, g, training=True, keep=None)
    eng.forward([p])
    torch.testing.assert_close(buf["feat"], o32(*args).detach(), **G.TOL)
    with pytest.raises(RuntimeError) as err:
        eng.backward(model, p, buf, torch.ones(3, 64))
    msg = str(err.value)
    assert "(max_degree + 1) * degree_embedding_size" in msg and "10240" in msg and "512" in msg and "31" in msg, msg
    assert "training-mode" not in msg
