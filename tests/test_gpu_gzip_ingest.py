"""Engine.count_fastq on ordinary .fastq.gz files with BC_GZ_DEVICE=all: the deflate stream is inflated on the device,
span by span, and the counts, rows and "Total sequences" are those of the same file read through zlib (BC_GZ_DEVICE=1,
the path every such file takes by default)."""
import os

import pytest

import bgzf
import gzip_ingest_files as files

pytestmark = pytest.mark.gpu


def count_file(plan, path):
    import ngs_barcode_count_amd as pkg
    eng = pkg.Engine(plan, device=0)
    try:
        total = eng.count_fastq(path)
        return total, eng.counters(), eng.result_rows(), eng.gz_blocks_inflated(), eng.gz_segments_inflated()
    finally:
        eng.close()


@pytest.fixture()
def small_spans(monkeypatch):
    for k, v in files.ENV.items():
        monkeypatch.setenv(k, v)
    return monkeypatch


@pytest.mark.parametrize("name", sorted(files.variants()))
def test_the_device_counts_what_zlib_counts(tmp_path, small_spans, name):
    from test_gpu_parity import make_plan
    plan = make_plan(files.case())
    path = files.write(tmp_path, name, files.variants()[name])
    small_spans.setenv("BC_GZ_DEVICE", "1")
    t_zlib, g_zlib, r_zlib, b_zlib, s_zlib = count_file(plan, path)
    small_spans.setenv("BC_GZ_DEVICE", "all")
    t_dev, g_dev, r_dev, b_dev, s_dev = count_file(plan, path)
    print(name, "total", t_dev, "segments", s_dev)
    assert (t_dev, g_dev, r_dev) == (t_zlib, g_zlib, r_zlib)
    assert t_zlib == files.N_READS + 1 and g_zlib["matched"] > files.N_READS // 2
    assert s_dev > 0 and s_zlib == 0 and (b_dev, b_zlib) == (0, 0)


def test_a_bgzf_file_still_takes_the_bgzf_path(tmp_path, small_spans):
    from test_gpu_parity import make_plan
    plan = make_plan(files.case())
    path = os.path.join(str(tmp_path), "blocked.fastq.gz")
    bgzf.write(path, files.text()[:400000], block_size=20000)
    small_spans.setenv("BC_GZ_DEVICE", "all")
    _, _, _, blocks, segments = count_file(plan, path)
    assert blocks > 0 and segments == 0


def test_a_damaged_trailer_crc_is_a_read_error(tmp_path, small_spans):
    import ngs_barcode_count_amd as pkg
    from test_gpu_parity import make_plan
    blob = bytearray(files.variants()["level_6"])
    blob[-6] ^= 0x04  # (the trailer is CRC32 then ISIZE: this is a CRC byte)
    path = files.write(tmp_path, "bad_crc", bytes(blob))
    small_spans.setenv("BC_GZ_DEVICE", "all")
    eng = pkg.Engine(make_plan(files.case()), device=0)
    with pytest.raises(pkg.BarcodeCountError) as err:
        eng.count_fastq(path)
    eng.close()
    assert err.value.code == pkg._lib.BC_ERR_INVALID
    assert "read error in " + path in str(err.value) and "file offset 0" in str(err.value) and "CRC32" in str(err.value)
