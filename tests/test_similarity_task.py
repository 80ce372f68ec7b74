"""python -m gcc_amd.tasks.similarity_search as a tool: files in a temporary folder, the reference-shaped result line,
--save-topk, and refusals by name."""
import ast
import os
import subprocess
import sys

import numpy as np
import pytest

from gcc_amd.tasks import similarity_search as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """two tiny networks that share 30 of their 40 authors; the second table is the first one's rows, noisily"""
    td = tmp_path_factory.mktemp("ss")
    rng = np.random.RandomState(3)
    emb = {}
    for net, first in (("neta", 0), ("netb", 10)):
        ids = rng.permutation(500)[:40] + 1
        lines = ["40 60"] + [f"{ids[a]} {ids[b]} {rng.randint(1, 3)}" for a, b in rng.randint(0, 40, (60, 2)) if a != b]
        (td / f"{net}.graph").write_text("\n".join(lines) + "\n")
        (td / f"{net}.dict").write_text("".join(f"Author {first + i}\t{ids[i]}\n" for i in range(40)))
        emb[net] = rng.randn(40, 16).astype(np.float32)
    da, db = (T.read_ss_graph(str(td / f"{n}.graph"), str(td / f"{n}.dict"))["name_dict"] for n in ("neta", "netb"))
    for name in set(da) & set(db):
        emb["netb"][db[name]] = emb["neta"][da[name]] + 0.7 * rng.randn(16).astype(np.float32)
    np.save(td / "a.npy", emb["neta"])
    np.savez(td / "b.npz", emb=emb["netb"])
    return td


def _argv(folder, *more):
    return ["--dataset", "neta_netb", "--data-root", str(folder), "--emb-path-1", str(folder / "a.npy"),
            "--emb-path-2", str(folder / "b.npz"), "--device", "cpu", *more]


def test_command_line_prints_the_reference_shaped_line(folder):
    run = subprocess.run([sys.executable, "-m", "gcc_amd.tasks.similarity_search", *_argv(folder, "--k", "1", "5")],
                         cwd=ROOT, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    line = run.stdout.strip().splitlines()[-1]
    assert line.startswith("{'Recall @ 1': ") and ", 'Recall @ 5': " in line
    result = ast.literal_eval(line)
    assert list(result) == ["Recall @ 1", "Recall @ 5", "queries"] and result["queries"] == 30
    assert 0.0 < result["Recall @ 1"] <= result["Recall @ 5"] <= 1.0
    assert result == T.main(_argv(folder, "--k", "1", "5"))


def test_save_topk_round_trips(folder, capsys):
    out = folder / "top.npz"
    result = T.main(_argv(folder, "--save-topk", str(out)))
    assert "Recall @ 20" in capsys.readouterr().out and list(result) == ["Recall @ 20", "Recall @ 40", "queries"]
    z = np.load(out)
    n = result["queries"]
    assert z["names"].shape == (n,) and z["topk_col"].shape == (n, 40) and z["topk_score"].shape == (n, 40)
    assert (z["topk_col"][:, :n] >= 0).all() and (z["topk_col"][:, n:] == -1).all() and np.isneginf(z["topk_score"][:, n:]).all()
    assert (z["topk_name"][:, 0] == z["names"][z["topk_col"][:, 0]]).all() and (z["topk_name"][:, n:] == "").all()
    assert (np.diff(z["topk_score"][:, :n], axis=1) <= 0).all()
    hit1 = z["topk_col"][:, 0] == z["target"]                    # the lists against the counts behind the printed line
    assert hit1.mean() == T.main(_argv(folder, "--k", "1"))["Recall @ 1"]


def test_missing_files_and_unknown_datasets_are_refused_by_name(folder):
    with pytest.raises(FileNotFoundError, match="unknown dataset 'neta_nope'.*nope.graph not found"):
        T.main(_argv(folder)[:1] + ["neta_nope"] + _argv(folder)[2:])
    with pytest.raises(ValueError, match="unknown dataset 'neta': expected <network 1>_<network 2>"):
        T.main(_argv(folder)[:1] + ["neta"] + _argv(folder)[2:])
    argv = _argv(folder)
    argv[argv.index("--emb-path-1") + 1] = str(folder / "absent.npy")
    with pytest.raises(FileNotFoundError, match="embedding file not found: .*absent.npy"):
        T.main(argv)
    np.save(folder / "flat.npy", np.zeros(5, np.float32))
    argv[argv.index("--emb-path-1") + 1] = str(folder / "flat.npy")
    with pytest.raises(ValueError, match="expected a \\[nodes, dim\\] table"):
        T.main(argv)
    with pytest.raises(ValueError, match="--k needs positive values"):
        T.main(_argv(folder, "--k", "0"))
