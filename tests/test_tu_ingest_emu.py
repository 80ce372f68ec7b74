"""gcc_text_ints_sep, gcc_tu_corpus, TUIngestEngine and DeviceGraphCorpus.from_device on the lock-step emulator against the host
reader and the host constructor: the checks of tests/tu_ingest_check.py.  (The emulator runs workgroups one after another: it sees
the kernels' logic at every seam, not a race between workgroups -- tests/test_tu_ingest_gpu.py makes every call twice for that.)"""
import re

import pytest

from tests import tu_ingest_check as C
from tests.hipemu.emu_driver import emu_lib
from tests.hipemu.emu_logreg import emu_ptr


@pytest.fixture(scope="module")
def tu():
    return C.Tu(emu_lib(), emu_ptr, "cpu")


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


def test_product_path_refuses_cpu_tensors(tmp_path):
    C.check_cpu_tensor_refused(emu_lib(), tmp_path)


def test_from_device_fills_the_members_of_the_host_constructor(tu, tmp_path):
    C.check_from_device(tu, tmp_path)


def test_write_tudataset_is_the_readers_inverse(tmp_path):
    C.check_write_tudataset(tmp_path)


def test_exported_constants_are_the_headers():
    from gcc_amd import _cabi

    src = open(_cabi.HEADER_PATH).read()
    for name in ("STATUS_TEXT_LINE_SHAPE", "STATUS_TU_DESCENDS", "STATUS_TU_GRAPH_COUNT", "STATUS_TU_BAD_ID", "STATUS_TU_SELF_LOOP",
                 "STATUS_TU_CROSS_GRAPH", "STATUS_TU_REPEATED", "STATUS_TU_ASYMMETRIC"):
        assert int(re.search(rf"#define GCC_{name} (\d+)", src).group(1)) == getattr(_cabi, name), name
