"""bc_bam_frame_device: the BAM record framing on the GPU, with no BGZF and no engine around it, over the texts of
bam_cases.py.  The device must report what the host build of the same logic reports (tests/bam/bam_host.cpp, under
sanitizers: run test_bam_emulation.py first), word for word -- status, end, candidates, and every record's offset,
length and flag -- and the writer's true offsets with it."""
import ctypes as C
import functools

import numpy as np
import pytest

import bam_cases

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def all_cases():
    return bam_cases.cases()


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    return dict(zip((c.name for c in all_cases()), bam_cases.run_host(all_cases(), tmp_path_factory.mktemp("bam_host"))))


def frame_on_device(c, guard=64):
    import torch
    import ngs_barcode_count_amd as pkg
    lib = pkg._lib.load()
    # the text sits at a 16-byte aligned address with marked bytes behind it; the record arrays have guard words as well
    buf = torch.full((len(c.text) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    if c.text:
        buf[:len(c.text)] = torch.from_numpy(np.frombuffer(c.text, dtype=np.uint8).copy()).cuda()
    out = torch.full((3, c.capacity + guard), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    res = pkg._lib.BamFrameResult()
    torch.cuda.synchronize()
    rc = lib.bc_bam_frame_device(0, None, buf.data_ptr(), len(c.text), c.start, c.n_ref, out[0].data_ptr(), out[1].data_ptr(),
                                 out[2].data_ptr(), c.capacity, C.byref(res))
    assert rc == 0, pkg._lib.last_error(lib)
    host = out.cpu().numpy().view(np.uint32)
    n = int(res.n_records)
    assert n <= c.capacity and (host[:, n:] == 0x5A5A5A5A).all(), c.name  # nothing written behind the records found
    assert bytes(buf[len(c.text):].cpu().numpy()) == b"\xA5" * 16
    recs = [tuple(int(host[k][i]) for k in range(3)) for i in range(n)]
    return int(res.status), int(res.n_candidates), int(res.end_pos), recs


def check(want, host_results):
    ran = 0
    for c in all_cases():
        if not want(c.name):
            continue
        got = frame_on_device(c)
        assert got == host_results[c.name][:4], c.name
        assert (got[0], got[2], got[3]) == (c.status, c.end_pos, c.records), c.name
        ran += 1
    return ran


def test_chains_lengths_names_and_flags(host_results):
    assert check(lambda n: n.startswith(("chain_", "l_seq", "names", "flags")), host_results) == 10


def test_headers_straddling_loads_scan_blocks_and_the_end_of_the_text(host_results):
    assert check(lambda n: n.startswith(("straddle_", "cut_")), host_results) == 72 + 38


def test_decoys_stay_unmarked(host_results):
    assert check(lambda n: n.startswith("decoy_"), host_results) == 6


def test_broken_chains_random_bytes_and_capacity(host_results):
    assert check(lambda n: n.startswith(("broken", "random", "record_too", "too_long", "capacity", "ref_id")), host_results) == 8


def test_arguments_that_contradict_each_other_are_refused():
    import torch
    import ngs_barcode_count_amd as pkg
    lib = pkg._lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    res = pkg._lib.BamFrameResult()
    ptr, o = buf.data_ptr(), out.data_ptr()
    for text, length, start, cap in [(ptr, 100, 101, 16), (ptr + 1, 100, 0, 16), (ptr, 100, 0, 0), (None, 100, 0, 16), (ptr, 1 << 31, 0, 16)]:
        assert lib.bc_bam_frame_device(0, None, text, length, start, 0, o, o, o, cap, C.byref(res)) == pkg._lib.BC_ERR_INVALID
    assert lib.bc_bam_frame_device(0, None, None, 0, 0, 0, o, o, o, 16, C.byref(res)) == 0  # an empty text is an empty chain
    assert (res.status, res.n_records, res.end_pos) == (0, 0, 0)
