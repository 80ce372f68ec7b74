"""Host side of GraphEncoder(gnn_model="gat"): the reference's state_dict keys and shapes, strict checkpoint loading, the
live-parameter helpers, the refusals, and the GAT kernels' footprint on gfx950 (no scratch, no spills)."""
import os
import shutil
import sys

import pytest
import torch

from gcc_amd.encoder import gat_params, grad_params
from tests.gat_check import gat_encoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_keys_and_shapes_are_the_references():
    enc = gat_encoder()
    sd = enc.state_dict()
    for i in range(5):
        assert sd[f"gnn.layers.{i}.gnn.fc.weight"].shape == (64, 49 if i == 0 else 64)
        assert sd[f"gnn.layers.{i}.gnn.attn_l"].shape == (1, 4, 16)
        assert sd[f"gnn.layers.{i}.gnn.attn_r"].shape == (1, 4, 16)
    assert sd["degree_embedding.weight"].shape == (513, 16)
    for k in range(3):
        assert sd[f"set2set.lstm.weight_ih_l{k}"].shape == (256, 128 if k == 0 else 64)
        assert sd[f"set2set.lstm.weight_hh_l{k}"].shape == (256, 64)
    assert sd["lin_readout.0.weight"].shape == (64, 128) and sd["lin_readout.2.weight"].shape == (64, 64)
    assert len(sd) == 5 * 3 + 1 + 3 * 4 + 4
    fresh = gat_encoder(seed=9)
    fresh.load_state_dict(sd, strict=True)
    assert all(torch.equal(fresh.state_dict()[k], v) for k, v in sd.items())


def test_initialisation_follows_gatconv_reset_parameters():
    """xavier_normal_(gain=calculate_gain('relu')) on fc.weight, attn_l, attn_r, after nn.Linear's own init, then the
    degree embedding, Set2Set's LSTM and lin_readout in the reference's order"""
    torch.manual_seed(0)
    gain = torch.nn.init.calculate_gain("relu")
    want = []
    for i in range(5):
        fc = torch.nn.Linear(49 if i == 0 else 64, 64, bias=False)
        al, ar = torch.empty(1, 4, 16), torch.empty(1, 4, 16)
        torch.nn.init.xavier_normal_(fc.weight, gain=gain)
        torch.nn.init.xavier_normal_(al, gain=gain)
        torch.nn.init.xavier_normal_(ar, gain=gain)
        want += [fc.weight, al, ar]
    emb = torch.nn.Embedding(513, 16)
    enc = gat_encoder(seed=0)
    got = [t for _, i, t in gat_params(enc) if _ in ("fc", "attn_l", "attn_r")]
    for a, b in zip(got, want):
        assert torch.equal(a.detach(), b.detach())
    assert torch.equal(enc.degree_embedding.weight.detach(), emb.weight.detach())


def test_every_gat_parameter_is_live():
    from gcc_amd.train_step import flatten_parameters

    enc = gat_encoder()
    assert {id(p) for _, _, p in grad_params(enc)} == {id(p) for p in enc.parameters()}
    flat, n_live = flatten_parameters(enc)
    assert n_live == flat.numel() == sum(p.numel() for p in enc.parameters())
    assert enc.bn_training() and not enc.eval().bn_training()


def test_model_gat_refuses_several_gpus(monkeypatch, tmp_path):
    import train

    args = train.parse_option(["--model", "gat", "--moco", "--model-path", str(tmp_path / "s"), "--tb-path", str(tmp_path / "t")])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="--model gat"):
        train.main(args)


sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_chains  # noqa: E402
from tests.test_solver_footprint import _metadata  # noqa: E402


@pytest.mark.skipif(not os.path.exists(isa_chains.HIPCC) or shutil.which("make") is None, reason="hipcc not installed")
@pytest.mark.parametrize("kernel", ["gat_forward_kernel", "gat_backward_kernel", "gat_wgrad_kernel", "gat_reduce_kernel"])
def test_gat_kernels_have_no_scratch(kernel):
    md = _metadata(isa_chains.isa_of(isa_chains.ROOT / "gcc_amd" / "csrc" / "gat.hip"), kernel)
    assert md["private_segment_fixed_size"] == 0, md
    assert md.get("vgpr_spill_count", 0) == 0, md
