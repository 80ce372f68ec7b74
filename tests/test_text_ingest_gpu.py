"""gcc_text_ints / gcc_text_line_ends and TextIngestEngine (gcc_amd/csrc/text_ingest.hip) on a real MI355X: the checks of
tests/text_ingest_check.py with every call made twice and the bits compared (only the device can show a race between workgroups),
the golden corpus through ``read_lscc`` and ``GraphBuildEngine.build``, and a generated file from its bytes to a sampled batch."""
import os

import numpy as np
import pytest

from tests import text_ingest_check as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ti():
    from gcc_amd import _cabi

    return C.Ti(_cabi.load(), _cabi.dev_ptr, "cuda:0", calls=2)


@pytest.mark.parametrize("name", sorted(C.SEAMS))
def test_tokens_at_the_seams_of_tile_wave_and_lane(ti, name):
    C.check_seam(ti, name)


@pytest.mark.parametrize("first", C.FIRST_BYTES)
def test_first_byte_cuts_a_token_of_its_own(ti, first):
    C.check_first_byte(ti, first)


@pytest.mark.parametrize("which", C.LENGTHS)
def test_text_lengths_around_a_tile_and_an_end_inside_a_token(ti, which):
    C.check_length(ti, which)


def test_scan_takes_a_second_pass(ti):
    C.check_scan_second_pass(ti)


def test_token_forms_and_the_edges_of_int32(ti):
    C.check_token_forms(ti)


def test_the_six_separators_and_no_others(ti):
    C.check_separators(ti)


@pytest.mark.parametrize("token", C.BAD_TOKENS, ids=[repr(t) for t in C.BAD_TOKENS])
def test_bad_token_sets_exactly_its_bit_and_its_offset(ti, token):
    C.check_bad_token(ti, token)


def test_lowest_of_three_bad_tokens_and_none_after_max_tokens(ti):
    C.check_lowest_bad_token(ti)


def test_counts_short_texts_and_record_shapes(ti):
    C.check_counts(ti)


def test_line_ends_at_tile_edges_and_past_the_last_line(ti):
    C.check_line_ends(ti)


@pytest.mark.parametrize("name", C.GOLDEN_FILES)
def test_read_lscc_of_the_golden_files_is_the_host_readers(ti, name):
    C.check_read_lscc_file(ti, os.path.join(C.GOLDEN, name))


@pytest.mark.parametrize("n", C.LSCC_SIZES)
def test_read_lscc_with_the_header_ending_in_different_tiles(ti, n, tmp_path):
    C.check_read_lscc_generated(ti, n, tmp_path)


def test_read_lscc_raises_the_host_readers_errors(ti, tmp_path):
    C.check_read_lscc_errors(ti, tmp_path)


def test_limits_short_workspace_capacity_and_null_members_are_refused_by_name(ti):
    C.check_refusals(ti)


def test_cpu_tensor_is_refused(ti, tmp_path):
    C.check_cpu_tensor_refused(ti.lib, tmp_path)


def test_upload_pads_with_zeros_around_the_chunk_size(ti, tmp_path):
    C.check_upload(ti, tmp_path)


def test_golden_files_build_the_reference_converters_graphs(ti):
    """read_lscc on the device, then gcc_graph_build, against the fixture the reference's own converter produced"""
    from gcc_amd.graph_build import GraphBuildEngine

    golden = np.load(os.path.join(C.GOLDEN, "x2dgl_golden.npz"))
    build = GraphBuildEngine(device="cuda:0")
    for name in C.GOLDEN_FILES:
        n, pairs = ti.engine.read_lscc(os.path.join(C.GOLDEN, name))
        assert pairs.is_cuda
        out = build.build(pairs, n)
        build.check_status(out)
        key = name[len("x2dgl_"):-len(".lscc")]
        assert np.array_equal(out["row_ptr"].cpu().numpy(), golden[f"{key}_row_ptr"]), name
        assert np.array_equal(out["col_idx"].cpu().numpy(), golden[f"{key}_col_idx"]), name


def test_file_to_batch_is_the_host_parsed_routes(tmp_path):
    """a generated file -> build_corpus(parse="device", keep_on_device=True) -> DeviceGraph.from_device -> one batch, bit-equal to
    the batch of the host-parsed route"""
    from gcc_amd.corpus import build_corpus
    from gcc_amd.graph import DeviceGraph
    from gcc_amd.graphgen import powerlaw_graph
    from gcc_amd.sampler import DeviceRWRSampler

    rp, ci = powerlaw_graph(2000, 12000)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    once = rows < ci                                                # every undirected edge once; the build inserts both directions
    lines = [f"vertices {n}\n"] + [f"{i} {i}\n" for i in range(n)] + [f"edges {int(once.sum())}\n"]
    lines += [f"{u} {v} 1\n" for u, v in zip(rows[once], ci[once])]
    (tmp_path / "powerlaw.lscc").write_text("".join(lines))
    batches = []
    for parse in ("device", "host"):
        (g,) = build_corpus(str(tmp_path), ["powerlaw.lscc"], device="cuda:0", keep_on_device=True, parse=parse)
        assert g["row_ptr"].is_cuda and g["counts"][0] == n
        graph = DeviceGraph.from_device(g["row_ptr"], g["col_idx"], rw_hops=16, validate="device")
        s = DeviceRWRSampler(graph, batch_size=8, run_seed=5)
        q, k = s.sample(0)
        s.check_status()
        batches.append((q.csr_numpy(), k.csr_numpy()))
    for a, b in zip(*batches):
        assert a["parent_nid"].size > 8
        for key in a:
            assert np.array_equal(a[key], b[key]), key
