"""gcc_text_ints / gcc_text_line_ends and TextIngestEngine (gcc_amd/csrc/text_ingest.hip) on the lock-step emulator against the host
reader: the checks of tests/text_ingest_check.py.  (The emulator runs workgroups one after another: it sees the kernels' logic at
every seam, not a race between workgroups -- tests/test_text_ingest_gpu.py makes every call twice for that.)"""
import os

import pytest

from tests import text_ingest_check as C
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_logreg import emu_ptr


@pytest.fixture(scope="module")
def ti():
    return C.Ti(emu_lib(), emu_ptr, "cpu")


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


def test_product_path_refuses_cpu_tensors(tmp_path):
    C.check_cpu_tensor_refused(emu_lib(), tmp_path)


def test_upload_pads_with_zeros_around_the_chunk_size(ti, tmp_path):
    C.check_upload(ti, tmp_path)


def test_exported_constants_are_the_headers():
    import re

    from gcc_amd import _cabi

    src = open(_cabi.HEADER_PATH).read()
    for name in ("TEXT_TILE_BYTES", "TEXT_SCAN_TILES", "TEXT_MAX_QUERIES", "STATUS_TEXT_NOT_INTEGER", "STATUS_TEXT_INT32_RANGE", "STATUS_TEXT_SHORT"):
        assert int(re.search(rf"#define GCC_{name} (\d+)", src).group(1)) == getattr(_cabi, name), name
