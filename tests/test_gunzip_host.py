"""The span inflater's lane code (csrc/bc_gunzip.h: find, measure, chain, decode, resolve) on the CPU, under
AddressSanitizer and UndefinedBehaviorSanitizer, over the scenarios of gunzip_cases.py at 1 KiB partitions: every
stream is zlib's (or written by hand where zlib's deflate never goes), the expected text is zlib's own, and a damaged
stream gives a status and no access outside a buffer.  test_gpu_gunzip.py runs the same scenarios on the device."""
import pytest

import gunzip_cases
import gunzip_lib

CASES = gunzip_cases.cases()


def test_the_case_table_holds_every_kind_of_stream():
    assert [n for n, _ in CASES] == [
        "level_1", "level_6", "level_9", "fixed_blocks", "stored_only", "sync_flush", "run_of_one_byte", "interrupted_runs",
        "far_distances", "stream_inside_a_stored_block", "cut_and_continue", "two_members", "one_byte_short", "damaged_header",
        "damaged_distance", "damaged_trailer"]


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_scenario_on_the_host(tmp_path, name):
    dict(CASES)[name](gunzip_lib.runner(tmp_path))
