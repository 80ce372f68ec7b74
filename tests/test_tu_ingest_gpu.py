"""gcc_text_ints_sep, gcc_tu_corpus, TUIngestEngine and DeviceGraphCorpus.from_device on a real MI355X: the checks of
tests/tu_ingest_check.py with every call made twice and the bits compared (only the device can show a race between workgroups), a
folder through ``GraphClassificationDatasetLabeled(corpus=...)`` to one batch, and ``generate.run`` on both parse routes."""
import numpy as np
import pytest
import torch

from tests import tu_ingest_check as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tu():
    from gcc_amd import _cabi

    return C.Tu(_cabi.load(), _cabi.dev_ptr, DEV, calls=2)


def test_both_knobs_off_is_the_old_entry_bit_for_bit(tu):
    C.check_knobs_off(tu)


def test_comma_forms_crlf_blank_lines_and_no_final_newline(tu):
    C.check_comma_forms(tu)


@pytest.mark.parametrize("name", sorted(C.SEAMS))
def test_comma_on_either_side_of_a_lane_wave_and_tile_seam(tu, name):
    C.check_comma_seam(tu, name)


def test_separator_run_with_its_newline_in_the_previous_tile(tu):
    C.check_newline_in_the_previous_tile(tu)


def test_line_records_lowest_offset_and_nothing_behind_max_tokens(tu):
    C.check_line_records(tu)


def test_count_only_call_without_an_output(tu):
    C.check_count_only(tu)


def test_extra_sep_that_is_a_digit_a_sign_or_a_separator_is_refused(tu):
    C.check_extra_sep_refused(tu)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_build_is_the_host_readers_corpus_in_any_line_order(tu, name, tmp_path):
    C.check_case(tu, name, tmp_path)


@pytest.mark.parametrize("name", sorted(C.ERRORS))
def test_errors_are_the_host_readers_first(tu, name, tmp_path):
    C.check_error(tu, name, tmp_path)


def test_status_word_steps_run_only_on_sound_input(tu):
    C.check_status_bits(tu)


def test_device_only_errors_name_the_file_and_the_offset(tu, tmp_path):
    C.check_device_only_errors(tu, tmp_path)


def test_limits_null_members_and_a_short_workspace_are_refused_by_name(tu):
    C.check_refusals(tu)


def test_from_device_fills_the_members_of_the_host_constructor(tu, tmp_path):
    C.check_from_device(tu, tmp_path)


def test_folder_to_a_labelled_batch_is_the_host_parsed_datasets(tu, tmp_path):
    from gcc_amd import ingest
    from gcc_amd.datasets import GraphClassificationDatasetLabeled

    pairs, indicator, labels = C.generated(seed=8, graphs=21)
    folder = C.write_files(tmp_path / "gen", pairs, indicator, labels, seed=41)
    kw = dict(rw_hops=16, positional_embedding_size=8, batch_size=8, device=DEV, edge_multiplicity=2)
    d = ingest.read_tudataset(folder, C.NAME)
    host = GraphClassificationDatasetLabeled(graphs=d["graphs"], labels=d["graph_labels"], batcher="device", **kw)
    got = tu.engine.read_tudataset(folder, C.NAME)
    dev = GraphClassificationDatasetLabeled(corpus=got["corpus"], **kw)
    assert dev.batcher == "device" and dev.graphs is None
    assert (dev.length, dev.node_cap, dev.num_classes) == (host.length, host.node_cap, host.num_classes) and len(dev) == 21
    assert np.array_equal(dev.sizes, host.sizes) and np.array_equal(dev.first, host.first) and np.array_equal(dev.labels, host.labels)
    idx = np.array([20, 3, 3, 0, 11], dtype=np.int64)
    (gh, lh), (gd, ld) = host.make_batch(idx), dev.make_batch(idx)
    host.check_status()
    dev.check_status()
    for name in ("node_off", "edge_off", "graph_id", "row_ptr", "col_idx", "seed_local"):
        assert torch.equal(getattr(gh, name), getattr(gd, name)), name
    assert torch.equal(lh, ld) and gh.valid == gd.valid == 5
    with pytest.raises(RuntimeError, match="_batch_of needs the host list graphs="):
        dev._batch_of([0])
    with pytest.raises(RuntimeError, match="_convert_idx needs the host list graphs="):
        dev._convert_idx(0)


def test_generate_run_writes_the_same_table_on_both_parse_routes(tmp_path):
    import train
    from gcc_amd.contrast import MemoryMoCo
    from gcc_amd.encoder import GraphEncoder
    from gcc_amd.tasks._common import checkpoint_table

    opt = train.parse_option(["--model-path", str(tmp_path / "saved"), "--tb-path", str(tmp_path / "tb"), "--moco", "--nce-k", "64",
                              "--rw-hops", "32", "--num-layer", "3", "--max-degree", "64"])
    torch.manual_seed(3)
    model = GraphEncoder(positional_embedding_size=32, max_node_freq=16, max_edge_freq=16, max_degree=64, freq_embedding_size=16,
                         degree_embedding_size=16, output_dim=64, node_hidden_dim=64, edge_hidden_dim=64, num_layers=3,
                         num_step_set2set=6, num_layer_set2set=3, norm=True, gnn_model="gin", degree_input=True)
    path = str(tmp_path / "toy.pth")
    torch.save({"opt": opt, "model": model.state_dict(), "contrast": MemoryMoCo(64, None, 64, 0.07, use_softmax=True).state_dict(),
                "optimizer": {}, "epoch": 1}, path)
    pairs, indicator, labels = C.generated(seed=9, graphs=19)
    folder = C.write_files(tmp_path / "gen", pairs, indicator, labels, seed=43)
    host = checkpoint_table(path, C.NAME, DEV, 8, tudataset=folder)
    dev = checkpoint_table(path, C.NAME, DEV, 8, tu_parse="device", tudataset=folder)
    assert host.shape == (19, 64) and host.dtype == dev.dtype and np.array_equal(host, dev)
