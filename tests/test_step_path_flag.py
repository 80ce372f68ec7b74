"""``train.py --step-path {auto,fused,api}``: parsing, routing and the refusals (CPU), and the fused step with
--optimizer sgd / adagrad through train.py and the fine-tuning main on a real MI355X."""
import os

import numpy as np
import pytest
import torch

from gcc_amd.train_step import resolve_step_path


def _route(step_path, optimizer="adam", gat=False, wide=False, moco=True, **kw):
    return resolve_step_path(step_path, optimizer=optimizer, gat=gat, wide=wide, moco=moco, **kw)


def test_step_path_defaults_to_auto_and_takes_three_values():
    import train

    assert train.parse_option([]).step_path == "auto"
    for v in ("auto", "fused", "api"):
        assert train.parse_option(["--step-path", v]).step_path == v
    with pytest.raises(SystemExit):
        train.parse_option(["--step-path", "eager"])


def test_auto_on_one_gpu_routes_every_command_line_as_before_the_flag():
    for moco in (False, True):
        assert _route("auto", "adam", moco=moco) == "fused"
        for opt in ("sgd", "adagrad"):
            assert _route("auto", opt, moco=moco) == "api"
        for opt in ("adam", "sgd", "adagrad"):
            assert _route("auto", opt, gat=True, moco=moco) == "api"
    assert _route("auto", "adam", wide=True, moco=True) == "fused"
    assert _route("auto", "adam", wide=True, moco=False) == "api"
    assert _route("auto", "sgd", wide=True, moco=True) == "api"
    assert _route("auto", "adam", finetune=True, moco=False) == "fused"
    assert _route("auto", "sgd", finetune=True, moco=False) == "api"
    assert _route("auto", "adam", finetune=True, wide=True, moco=False) == "api"


def test_auto_on_several_ranks_takes_the_fused_step_for_every_optimizer():
    for opt in ("adam", "sgd", "adagrad"):
        assert _route("auto", opt, world=2) == "fused"
        assert _route("auto", opt, wide=True, world=2) == "fused"
    with pytest.raises(NotImplementedError, match="--model gat.*one GPU"):
        _route("auto", "adam", gat=True, world=2)
    with pytest.raises(NotImplementedError, match="--step-path api.*one GPU"):
        _route("api", "adam", world=2)


def test_fused_and_api_are_honoured_for_every_optimizer():
    for opt in ("adam", "sgd", "adagrad"):
        assert _route("fused", opt) == _route("fused", opt, moco=False) == _route("fused", opt, wide=True) == "fused"
        assert _route("fused", opt, finetune=True, moco=False) == "fused"
        assert _route("api", opt) == _route("api", opt, gat=True) == _route("api", opt, finetune=True, moco=False) == "api"


def test_fused_is_refused_by_name_where_there_is_no_fused_step(tmp_path):
    import train

    with pytest.raises(NotImplementedError, match="--step-path fused.*--model gat.*API path"):
        _route("fused", "sgd", gat=True)
    with pytest.raises(NotImplementedError, match="--step-path fused.*--hidden-size above 64 without --moco.*API path"):
        _route("fused", "adam", wide=True, moco=False)
    with pytest.raises(NotImplementedError, match="--step-path fused.*--finetune with --hidden-size above 64.*API path"):
        _route("fused", "adam", wide=True, moco=False, finetune=True)
    # the same through train.py's main, before any device work
    common = ["--model-path", str(tmp_path / "s"), "--tb-path", str(tmp_path / "t"), "--step-path", "fused"]
    for flags, text in ((["--model", "gat", "--moco"], "--model gat"), (["--hidden-size", "128"], "--hidden-size above 64 without --moco"),
                        (["--finetune", "--hidden-size", "128", "--dataset", "imdb-binary"], "--finetune with --hidden-size above 64")):
        args = train.parse_option(common + flags)
        args.gpu = 0
        with pytest.raises(NotImplementedError, match=f"--step-path fused.*{text}"):
            train.main(args)


# ------------------------------------------------------------------------------------------------------------ on the device
def _corpus(tmp_path):
    """the toy corpus of tests/test_train_main_gpu.py"""
    from gcc_amd import ingest
    from gcc_amd.graphgen import powerlaw_graph

    gs = [powerlaw_graph(20000, 200000, 0), powerlaw_graph(6000, 50000, 1), powerlaw_graph(2500, 20000, 2)]
    sizes = np.array([len(rp) - 1 for rp, _ in gs], dtype=np.int64)
    path = tmp_path / "small.bin"
    ingest.write_dgl_graphs(str(path), gs, labels={"graph_sizes": sizes})
    return str(path)


def _flat_state(ckpt, key):
    """the checkpoint's ``optimizer`` is a flat optimizer's: one state tensor over the live parameters, torch's param_groups"""
    st = ckpt["optimizer"]["state"]
    assert set(st) == {"step", key} and st[key].dim() == 1 and st[key].numel() > 50000 and st["step"] > 0
    assert torch.isfinite(st[key]).all() and float(st[key].abs().max()) > 0
    return ckpt["optimizer"]["param_groups"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("flags,cls,key", [
    (["--moco", "--optimizer", "sgd", "--nce-k", "256"], "MoCoTrainStep", "momentum_buffer"),
    (["--optimizer", "adagrad", "--nce-k", "31"], "E2ETrainStep", "sum"),
])
def test_fused_step_path_through_train_py(tmp_path, monkeypatch, capsys, flags, cls, key):
    import train

    made = []

    class Recorded(getattr(train, cls)):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(train, cls, Recorded)
    argv = ["--exp", "P", "--model-path", str(tmp_path / "s"), "--tb-path", str(tmp_path / "t"), "--gpu", "0", "--batch-size", "32",
            "--num-workers", "2", "--num-copies", "1", "--num-samples", "128", "--rw-hops", "64", "--dgl-file", _corpus(tmp_path),
            "--epochs", "2", "--print-freq", "4", "--tb-freq", "1000", "--producer-lanes", "2", "--producer-chunk", "2",
            "--step-path", "fused"]
    args = train.parse_option(argv + flags)
    args.gpu = args.gpu[0]
    loss = train.main(args)
    out = capsys.readouterr().out
    assert len(made) == 1 and made[0].optimizer.steps == 16 and made[0].optimizer.rule == args.optimizer      # 2 x 8 steps
    vals = [float(ln.split("loss ")[1].split(" ")[0]) for ln in out.splitlines() if ln.startswith("Train:")]
    assert len(vals) == 4 and all(np.isfinite(v) and 0.0 < v < 7.0 for v in vals) and np.isfinite(loss), vals
    ckpt = torch.load(os.path.join(args.model_folder, "current.pth"), map_location="cpu", weights_only=False)
    assert set(ckpt) == {"opt", "model", "contrast", "optimizer", "epoch"} | ({"model_ema"} if "--moco" in flags else set())
    assert ckpt["epoch"] == 2 and ckpt["opt"].step_path == "fused"
    group = _flat_state(ckpt, key)
    assert set(group) == ({"lr", "momentum", "weight_decay"} if key == "momentum_buffer" else {"lr", "lr_decay", "eps", "weight_decay"})


@pytest.mark.gpu
def test_fused_step_path_through_the_finetune_main(tmp_path, monkeypatch, capsys):
    import train
    from gcc_amd import finetune
    from gcc_amd.graphgen import powerlaw_graph

    rps, cis = zip(*[powerlaw_graph(12 + (i % 7) * 3, 40 + (i % 5) * 10, 100 + i) for i in range(60)])
    node_off = np.concatenate([[0], np.cumsum([len(rp) - 1 for rp in rps])])
    edge_base = np.concatenate([[0], np.cumsum([len(ci) for ci in cis])])
    npz = tmp_path / "graphs.npz"
    np.savez(npz, node_off=node_off, row_ptr=np.concatenate([[0]] + [rp[1:] + edge_base[i] for i, rp in enumerate(rps)]),
             col_idx=np.concatenate(cis), graph_labels=np.arange(60) % 3)
    made = []

    class Recorded(finetune.FinetuneTrainStep):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(finetune, "FinetuneTrainStep", Recorded)
    args = train.parse_option(["--finetune", "--dataset", "imdb-binary", "--epochs", "2", "--batch-size", "16", "--graphs-npz", str(npz),
                               "--gpu", "0", "--optimizer", "sgd", "--step-path", "fused", "--num-layer", "3", "--max-degree", "64",
                               "--rw-hops", "32", "--model-path", str(tmp_path / "s"), "--tb-path", str(tmp_path / "t")])
    args.gpu = args.gpu[0]
    f1 = train.main(args)
    out = capsys.readouterr().out
    assert len(made) == 1 and made[0].optimizer.rule == "sgd" and made[0].optimizer.steps == made[0].head_optimizer.steps > 0
    assert "betas" in made[0].head_optimizer.param_groups[0]                     # the head's optimizer stays Adam
    assert 0.0 <= f1 <= 1.0 and "Epoch 2, loss" in out and "nan" not in out.split("Epoch 2, loss")[1][:12]
    folder = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "s") for f in fs if f == "current.pth"]
    ckpt = torch.load(folder[0], map_location="cpu", weights_only=False)
    assert set(ckpt) == {"opt", "model", "contrast", "optimizer", "epoch"} and ckpt["epoch"] == 2
    st = ckpt["optimizer"]["state"]
    assert set(st) == {"step", "momentum_buffer"} and st["momentum_buffer"].dim() == 1 and float(st["momentum_buffer"].abs().max()) > 0
    assert set(ckpt["optimizer"]["param_groups"][0]) == {"lr", "momentum", "weight_decay"}
