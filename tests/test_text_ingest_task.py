"""``python -m gcc_amd.x2dgl --parse device`` and ``train.py --graph-parse`` (CPU tier, the emulator's engines injected): the device
parser writes the same corpus as the host parser, and both flags default to ``host`` and refuse what they cannot serve by name."""
import os
import shutil

import pytest

from gcc_amd import x2dgl
from gcc_amd.graph_build import GraphBuildEngine
from gcc_amd.text_ingest import TextIngestEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("x2dgl_tie.lscc", "x2dgl_hub.lscc", "x2dgl_small.lscc")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("text_ingest_task")
    for name in FILES:
        shutil.copy(os.path.join(GOLDEN, name), root / name)
    return root


def engines():
    from tests.hipemu.emu_driver import emu_lib
    from tests.hipemu.emu_logreg import emu_ptr

    return dict(engine=GraphBuildEngine(emu_lib(), emu_ptr, "cpu"), text_engine=TextIngestEngine(emu_lib(), emu_ptr, "cpu"))


def test_device_parse_writes_the_host_parsers_bytes(folder, tmp_path, caplog):
    argv = ["--graph-dir", str(folder), "--files", ",".join(FILES), "--device", "cpu", "--save-file"]
    with caplog.at_level("INFO", logger="gcc_amd.x2dgl"):
        host = x2dgl.main(argv + [str(tmp_path / "host.bin"), "--parse", "host"])
    def lines():
        return [r.getMessage() for r in caplog.records if not r.getMessage().startswith("save graphs to")]

    host_log = lines()
    caplog.clear()
    with caplog.at_level("INFO", logger="gcc_amd.x2dgl"):
        dev = x2dgl.main(argv + [str(tmp_path / "dev.bin"), "--parse", "device"], **engines())
    assert lines() == host_log and len(host_log) == 9       # the same lines on both routes
    assert (tmp_path / "host.bin").read_bytes() == (tmp_path / "dev.bin").read_bytes()
    assert [g["name"] for g in dev] == [g["name"] for g in host]
    x2dgl.main(argv + [str(tmp_path / "default.bin")])
    assert (tmp_path / "default.bin").read_bytes() == (tmp_path / "host.bin").read_bytes()


def test_device_parse_keeps_the_converters_refusals(folder, tmp_path):
    common = ["--graph-dir", str(folder), "--save-file", str(tmp_path / "x.bin"), "--device", "cpu", "--parse", "device"]
    with pytest.raises(SystemExit, match="no graph file to convert"):
        x2dgl.main(common, **engines())
    with pytest.raises(SystemExit, match="nope.lscc"):
        x2dgl.main(common + ["--files", "nope.lscc"], **engines())
    (tmp_path / "loops.lscc").write_text("v 2\n0 5\n1 6\ne 2\n0 0 1\n1 1 1\n")
    with pytest.raises(SystemExit, match="no edge is left in loops.lscc"):
        x2dgl.main(["--graph-dir", str(tmp_path), "--save-file", str(tmp_path / "x.bin"), "--device", "cpu", "--parse", "device",
                    "--files", "loops.lscc"], **engines())


def test_device_parse_on_the_cpu_without_engines_is_refused_by_name(folder, tmp_path, capsys):
    with pytest.raises(SystemExit):
        x2dgl.main(["--graph-dir", str(folder), "--save-file", str(tmp_path / "x.bin"), "--device", "cpu", "--parse", "device",
                    "--files", ",".join(FILES)])
    assert "--parse device parses on the device: not with --device cpu" in capsys.readouterr().err
    assert not (tmp_path / "x.bin").exists()


def test_train_refuses_graph_parse_without_graph_dir(capsys):
    import train

    with pytest.raises(SystemExit):
        train.parse_option(["--graph-parse", "device"])
    assert "--graph-parse says where the files of --graph-dir are parsed" in capsys.readouterr().err
    opt = train.parse_option(["--graph-dir", "somewhere", "--graph-parse", "device"])
    assert opt.graph_parse == "device" and opt.graph_dir == "somewhere"


def test_both_defaults_are_the_host_reader(folder, tmp_path, monkeypatch):
    import train
    from gcc_amd import corpus, ingest

    assert train.parse_option([]).graph_parse == "host" and train.parse_option(["--graph-dir", "d"]).graph_parse == "host"
    seen = []
    real = ingest.read_lscc
    monkeypatch.setattr(ingest, "read_lscc", lambda path: seen.append(path) or real(path))
    x2dgl.main(["--graph-dir", str(folder), "--files", FILES[0], "--device", "cpu", "--save-file", str(tmp_path / "a.bin")])
    corpus.build_corpus(str(folder), [FILES[1]], device="cpu")
    corpus.build_graph(str(folder / FILES[2]), device="cpu")
    assert [os.path.basename(p) for p in seen] == list(FILES)
