"""bc_gunzip_span_device on the GPU over the scenarios of gunzip_cases.py, every one of which has gone through the host
build of the same lane code under sanitizers (test_gunzip_host.py) -- run that one first.  The text is zlib's byte for
byte (the scenarios assert it), and every result field is the one the host build gives for the same span."""
import ctypes as C

import numpy as np
import pytest

import gunzip_cases
import gunzip_lib

pytestmark = pytest.mark.gpu

CASES = gunzip_cases.cases()


def device_runner(tmp_path):
    import torch
    import ngs_barcode_count_amd as pkg
    lib = pkg._lib.load()
    host = gunzip_lib.runner(tmp_path)

    def run(src, start_bit, hist, capacity, part_bytes):
        d_src = torch.from_numpy(np.frombuffer(src + b"\0", dtype=np.uint8).copy()).cuda()  # (never an empty tensor)
        d_hist = torch.from_numpy(np.frombuffer(hist, dtype=np.uint8).copy()).cuda() if hist else None
        d_text = torch.full((capacity + 1,), 0xAA, dtype=torch.uint8, device="cuda")
        res = pkg._lib.GunzipResult()
        torch.cuda.synchronize()
        rc = lib.bc_gunzip_span_device(0, None, d_src.data_ptr(), len(src), start_bit, d_hist.data_ptr() if hist else None,
                                       d_text.data_ptr(), capacity, part_bytes, C.byref(res))
        assert rc == 0, pkg._lib.last_error(lib)
        image = d_text.cpu().numpy().tobytes()
        assert image[capacity:] == b"\xAA"  # nothing past the capacity
        got = gunzip_cases.Result(*[getattr(res, f) for f in gunzip_cases.Result._fields])
        want, want_image = host(src, start_bit, hist, capacity, part_bytes)
        assert got == want, (got, want)
        assert image[:capacity] == want_image
        return got, image[:capacity]
    return run


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_scenario_on_the_device(tmp_path, name):
    dict(CASES)[name](device_runner(tmp_path))


def test_arguments_that_contradict_each_other_are_refused():
    import torch
    import ngs_barcode_count_amd as pkg
    lib = pkg._lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    res = pkg._lib.GunzipResult()
    for src_bytes, start_bit, part in [(4096, 8 * 4096 + 1, 1024), (4096, 0, 100), (4096, 0, 8), (1 << 28, 0, 1024)]:
        rc = lib.bc_gunzip_span_device(0, None, buf.data_ptr(), src_bytes, start_bit, None, buf.data_ptr(), 4096, part, C.byref(res))
        assert rc == pkg._lib.BC_ERR_INVALID, (src_bytes, start_bit, part)
