"""``python -m gcc_amd.x2dgl`` on the three files of tests/golden (CPU tier): ``--device cpu`` and the emulator library injected
write the same corpus; it reads back through ``ingest.read_dgl_graphs(validate=True)``, is ordered by node count descending with
ties by file name, and ``--save-npz`` round-trips."""
import os
import shutil

import numpy as np
import pytest

from gcc_amd import ingest, x2dgl
from gcc_amd.graph_build import GraphBuildEngine
from gcc_amd.graphgen import check_contract

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("x2dgl_tie.lscc", "x2dgl_hub.lscc", "x2dgl_small.lscc")
ORDER = ("x2dgl_hub.lscc", "x2dgl_small.lscc", "x2dgl_tie.lscc")            # 87 nodes, then the two of 5 by name


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("x2dgl")
    for name in FILES:
        shutil.copy(os.path.join(GOLDEN, name), root / name)
    return root


def emu_engine():
    from tests.hipemu.emu_driver import emu_lib
    from tests.hipemu.emu_logreg import emu_ptr

    return GraphBuildEngine(emu_lib(), emu_ptr, "cpu")


@pytest.mark.parametrize("how", ["cpu", "emulator"])
def test_corpus_reads_back_in_the_documented_order(folder, how, caplog):
    golden = np.load(os.path.join(GOLDEN, "x2dgl_golden.npz"))
    out, npz = folder / f"{how}.bin", folder / f"npz_{how}"
    argv = ["--graph-dir", str(folder), "--save-file", str(out), "--files", ",".join(FILES), "--embed-dim", "64", "--save-npz", str(npz)]
    with caplog.at_level("INFO", logger="gcc_amd.x2dgl"):
        written = x2dgl.main(argv + ["--device", "cpu"], engine=emu_engine() if how == "emulator" else None)
    assert [g["name"] for g in written] == list(ORDER)
    graphs, labels = ingest.read_dgl_graphs(str(out), validate=True)
    sizes = labels["graph_sizes"]
    assert sizes.dtype == np.int64 and sizes.tolist() == [87, 5, 5] and (np.diff(sizes) <= 0).all()
    for (rp, ci), name in zip(graphs, ORDER):
        check_contract(rp, ci)
        key = name[len("x2dgl_"):-len(".lscc")]
        assert np.array_equal(rp, golden[f"{key}_row_ptr"]) and np.array_equal(ci, golden[f"{key}_col_idx"])
        z = np.load(npz / (name + ".npz"))
        assert z["row_ptr"].dtype == np.int32 and np.array_equal(z["row_ptr"], rp) and np.array_equal(z["col_idx"], ci)
    # the reference's own log line, two slots per self-loop line
    assert "5 nodes, 10 edges, 6 self-loop(s) removed, 4 zero-degree node(s) removed" in caplog.text
    assert "87 nodes, 260 edges, 2 self-loop(s) removed, 9 zero-degree node(s) removed" in caplog.text


def test_both_paths_write_the_same_bytes(folder, tmp_path):
    argv = ["--graph-dir", str(folder), "--files", ",".join(FILES), "--device", "cpu", "--save-file"]
    x2dgl.main(argv + [str(tmp_path / "cpu.bin")])
    x2dgl.main(argv + [str(tmp_path / "emu.bin")], engine=emu_engine())
    assert (tmp_path / "cpu.bin").read_bytes() == (tmp_path / "emu.bin").read_bytes()


def test_default_names_are_the_references_and_a_missing_file_is_refused(folder, tmp_path):
    with pytest.raises(SystemExit, match="no graph file to convert"):
        x2dgl.main(["--graph-dir", str(folder), "--save-file", str(tmp_path / "x.bin"), "--device", "cpu"])
    with pytest.raises(SystemExit, match="nope.lscc"):
        x2dgl.main(["--graph-dir", str(folder), "--save-file", str(tmp_path / "x.bin"), "--device", "cpu", "--files", "nope.lscc"])
    shutil.copy(folder / "x2dgl_small.lscc", tmp_path / x2dgl.REFERENCE_FILES[2])
    written = x2dgl.main(["--graph-dir", str(tmp_path), "--save-file", str(tmp_path / "y.bin"), "--device", "cpu"])
    assert [g["name"] for g in written] == [x2dgl.REFERENCE_FILES[2]]
    assert ingest.read_dgl_labels(str(tmp_path / "y.bin"))["graph_sizes"].tolist() == [5]


def test_truncated_file_is_refused_by_name(tmp_path):
    text = open(os.path.join(GOLDEN, "x2dgl_small.lscc")).read().splitlines(keepends=True)
    cut = tmp_path / "cut.lscc"
    cut.write_text("".join(text[:-2]))                                  # two edge lines short
    with pytest.raises(ValueError, match="cut.lscc: truncated: 11 edge lines"):
        ingest.read_lscc(str(cut))
    cut.write_text("".join(text[:5]))                                   # ends inside the vertex lines
    with pytest.raises(ValueError, match="cut.lscc: truncated: 9 vertex lines"):
        ingest.read_lscc(str(cut))
    cut.write_text("".join(text[:-1]) + "3 x 1\n")
    with pytest.raises(ValueError, match="other than integers"):
        ingest.read_lscc(str(cut))
