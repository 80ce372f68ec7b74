"""python -m gcc_amd.tasks.similarity_search --load-path: both co-author networks are embedded with the checkpoint (the
weighted networks as multigraphs, generate.py's --ss-graph path) and searched without a trip through disk.  Kernels on
the emulator (generate.py's pipeline seam); the result equals evaluate() on the tables generate.py writes."""
import argparse
import os

import numpy as np
import pytest

from gcc_amd.tasks import similarity_search as T
from tests.test_wide_resident_emu import EmuPipeline, write_checkpoint


class MultigraphEmuPipeline(EmuPipeline):
    """EmuPipeline whose parent graph carries no contract bit when the dataset is a multigraph (as DeviceGraph does)"""

    def node_dataset(self, **kw):
        import torch

        from gcc_amd.datasets import NodeClassificationDataset
        from gcc_amd.graph import max_nodes_out_degree_table
        from tests.hipemu.emu_driver import EmuGraph, emu_sample_batch
        from tests.hipemu.emu_encoder import CpuBatch

        (rp, ci), mult, B = kw["graph"], kw["edge_multiplicity"], kw["batch_size"]
        assert kw.get("multigraph") is True
        g = EmuGraph(rp, ci, rw_hops=kw["rw_hops"], restart_prob=kw["restart_prob"], contract_checked=False,
                     ltab=max_nodes_out_degree_table(int(np.diff(rp).max()), kw["rw_hops"], kw["restart_prob"], mult))
        self.node_cap = B * (g.lmax + 1)

        def sample_fn(first_id, seeds):
            res, status, used = emu_sample_batch(g, B, kw["run_seed"], first_id, seeds=seeds, edge_cap=8 * B * (g.lmax + 1) ** 2)
            assert status == 0 and (used == seeds).all()
            out = []
            for r in res:
                n = len(r["parent_nid"])
                out.append(CpuBatch(dict(node_off=torch.from_numpy(r["node_off"].astype(np.int64)),
                                         row_ptr=torch.from_numpy(r["row_ptr"].astype(np.int64)),
                                         col_idx=torch.from_numpy(r["col_idx"].astype(np.int64)),
                                         pos_undirected=torch.zeros(n, 32)), node_cap=self.node_cap))
            return tuple(out)

        return NodeClassificationDataset(sample_fn=sample_fn, **kw), self.node_cap, lambda: None


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """two toy weighted networks (24 authors each, weights 1..4) that share 18 author names"""
    td = tmp_path_factory.mktemp("ssg")
    rng = np.random.RandomState(4)
    for net, first in (("neta", 0), ("netb", 6)):
        n = 24
        ids = rng.permutation(300)[:n] + 1
        pairs = {(i, i + 1) for i in range(n - 1)}
        while len(pairs) < 2 * n:
            a, b = sorted(rng.randint(0, n, 2))
            if a != b:
                pairs.add((a, b))
        lines = [f"{n} {len(pairs)}"] + [f"{ids[a]} {ids[b]} {rng.randint(1, 5)}" for a, b in sorted(pairs)]
        (td / f"{net}.graph").write_text("\n".join(lines) + "\n")
        (td / f"{net}.dict").write_text("".join(f"Author {first + i}\t{ids[i]}\n" for i in range(n)))
    return td


def test_load_path_equals_evaluate_on_the_tables_generate_writes(folder, tmp_path, capsys):
    import generate

    load_path, opt = write_checkpoint(tmp_path, 96)
    argv = ["--dataset", "neta_netb", "--data-root", str(folder), "--device", "cpu", "--k", "1", "5", "--batch-size", "16"]
    from gcc_amd.simsearch import SimilarityEngine
    from tests.hipemu.emu_driver import emu_lib

    eng = SimilarityEngine(lib=emu_lib(), ptr=lambda t: 0 if t is None else t.data_ptr())      # gcc_sim_search on the emulator
    result = T.main(argv + ["--load-path", load_path, "--save-emb", str(tmp_path / "emb")], pipeline=MultigraphEmuPipeline(),
                    engine=eng)
    assert list(result) == ["Recall @ 1", "Recall @ 5", "queries"] and result["queries"] == 18
    assert capsys.readouterr().out.strip().splitlines()[-1] == str(result)          # the same result line
    # generate.py on each network, same checkpoint (same seed): the tables it writes
    tables = []
    for net in ("neta", "netb"):
        a = argparse.Namespace(load_path=load_path, dataset=net, gpu=None, edgelist=None, nodelabel=None,
                               ss_graph=str(folder / f"{net}.graph"), ss_dict=None, graph_npz=None, graphs_npz=None, tudataset=None,
                               edge_multiplicity=0, batch_size=16, wide_eval="chain")
        generate.main(a, pipeline=MultigraphEmuPipeline())
        tables.append(np.load(os.path.join(opt.model_folder, net + ".npy")))
        assert tables[-1].shape == (24, 96)
        assert np.array_equal(tables[-1], np.load(tmp_path / "emb" / f"{net}.npy"))  # --save-emb stored what was searched
    dict_1, dict_2 = T.load_dicts(str(folder), "neta_netb")
    want, _ = T.evaluate(tables[0], tables[1], dict_1, dict_2, ks=(1, 5), device="cpu")
    assert result == want
    got, _ = T.evaluate(tables[0], tables[1], dict_1, dict_2, ks=(1, 5), device="cpu", engine=eng)
    assert got == want


def test_paths_are_optional_only_with_a_checkpoint(folder):
    with pytest.raises(SystemExit):
        T.main(["--dataset", "neta_netb", "--data-root", str(folder), "--device", "cpu"])
