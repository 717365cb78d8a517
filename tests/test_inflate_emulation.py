"""The device inflater's decoder (csrc/bc_inflate.h) on the host, under AddressSanitizer and UndefinedBehaviorSanitizer:
every table the GPU test (test_gpu_inflate.py) sends to the device, the damaged ones included, goes through the same
code here first.  A good block must equal zlib's output, a damaged one must be flagged, and the sanitizers must stay
silent: the decoder may never touch a byte outside the block's own stream and text, whatever the stream says."""
import functools

import pytest

import inflate_cases
import inflate_lib


@functools.lru_cache(maxsize=None)
def all_cases():
    return inflate_cases.cases()


def run_group(tmp_path, want):
    ran = 0
    for name, blocks in all_cases():
        if not want(name, blocks):
            continue
        table, status, dst = inflate_lib.run(blocks, tmp_path, name)
        inflate_cases.check(name, blocks, table, status, dst)
        # nothing outside the blocks' own output ranges was written
        image = bytearray(dst)
        for _, dst_off, _, isize, _ in table:
            image[dst_off:dst_off + isize] = b"\xAA" * isize
        assert bytes(image) == b"\xAA" * len(image), name
        ran += 1
    return ran


def is_good(blocks):
    return all(b[3] is not None for b in blocks)


def test_good_blocks_equal_zlib(tmp_path):
    assert run_group(tmp_path, lambda name, blocks: is_good(blocks)) >= 13


def test_damaged_blocks_are_flagged_and_their_neighbours_come_out_right(tmp_path):
    assert run_group(tmp_path, lambda name, blocks: not is_good(blocks) and not name.startswith("bit_flip")) >= 9


def test_every_single_bit_flip_is_flagged(tmp_path):
    assert run_group(tmp_path, lambda name, blocks: name.startswith("bit_flip")) == 32


def test_status_says_what_was_wrong(tmp_path):
    want = {"wrong_crc": 7, "isize_too_small": 5, "isize_too_large": 6, "payload_cut_short": 4, "payload_empty": 4, "btype3": 1,
            "stored_len_nlen": 1, "distance_before_start": 3, "distance_before_start_far": 3}
    got = {}
    for name, blocks in all_cases():
        if name in want:
            _, status, _ = inflate_lib.run(blocks, tmp_path, name)
            got[name] = status[1]
    assert got == want
