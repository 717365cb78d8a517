"""The BGZF index (bc_bgzf_scan) and where a shard of a BGZF file begins (bc_fastq_gz_record_start): host logic only."""
import ctypes as C
import gzip
import random
import struct

import pytest

import bgzf
import inflate_cases


@pytest.fixture(scope="module")
def lib():
    import ngs_barcode_count_amd as pkg
    return pkg._lib.load()


def scan(lib, path):
    n, size = C.c_uint64(), C.c_uint64()
    rc = lib.bc_bgzf_scan(str(path).encode(), C.byref(n), C.byref(size))
    return rc, n.value, size.value


TEXT = inflate_cases.fastq_text(200_000, seed=11)


@pytest.mark.parametrize("block_size", [300, 700, 4096, 65280])
@pytest.mark.parametrize("eof_marker", [True, False])
def test_scan_accepts_the_writers_files(lib, tmp_path, block_size, eof_marker):
    p = tmp_path / "a.fastq.gz"
    bgzf.write(p, TEXT, block_size=block_size, eof_marker=eof_marker)
    assert gzip.decompress(p.read_bytes()) == TEXT
    n_text = -(-len(TEXT) // block_size)
    assert scan(lib, p) == (0, n_text + (1 if eof_marker else 0), len(TEXT))


def test_scan_accepts_an_empty_member_in_the_middle_and_other_subfields(lib, tmp_path):
    p = tmp_path / "b.fastq.gz"
    parts = [bgzf.member(TEXT[:1000]), bgzf.EOF_MARKER, bgzf.member(TEXT[1000:3000], extra_before=b"XY" + struct.pack("<H", 3) + b"abc"),
             bgzf.member(TEXT[3000:3001], extra_after=b"ZZ" + struct.pack("<H", 0)), bgzf.member(b""), bgzf.EOF_MARKER]
    p.write_bytes(b"".join(parts))
    assert gzip.decompress(p.read_bytes()) == TEXT[:3001]
    assert scan(lib, p) == (0, 6, 3001)


def test_scan_refuses_what_is_not_bgzf(lib, tmp_path):
    import ngs_barcode_count_amd as pkg
    good = bgzf.compress(TEXT[:50_000], block_size=4096)
    plain_member = gzip.compress(TEXT[:500])
    oversize = bgzf.member(TEXT[:100], isize=65537)
    past_eof = bytearray(bgzf.member(TEXT[:100]))
    struct.pack_into("<H", past_eof, 16, len(past_eof) + 10)
    files = {
        "gzip_open": None,
        "prefix_then_plain_member": good + plain_member,
        "bsize_past_eof": good + bytes(past_eof),
        "cut_inside_a_block": good[:len(good) - 28 - 40],
        "isize_above_65536": good + oversize,
        "not_gzip": TEXT[:5000],
    }
    for name, blob in files.items():
        p = tmp_path / (name + ".fastq.gz")
        if blob is None:
            with gzip.open(p, "wb") as f:
                f.write(TEXT[:50_000])
        else:
            p.write_bytes(blob)
        rc, n, size = scan(lib, p)
        assert (rc, n, size) == (pkg._lib.BC_ERR_UNSUPPORTED, 0, 0), name
        assert "not BGZF" in pkg._lib.last_error(lib), name
    assert scan(lib, tmp_path / "missing.fastq.gz")[0] == pkg._lib.BC_ERR_INVALID


def test_gz_record_start_equals_the_plain_files_at_every_offset(lib, tmp_path):
    rng = random.Random(5)
    recs = []
    for i in range(60):
        n = rng.randint(1, 90)
        qual = "".join(rng.choice("@+IF#5") for _ in range(n))
        if i % 3 == 0:
            qual = "@" + qual[1:]  # a quality line that looks like a header
        if i % 7 == 0:
            qual = "+" + qual[1:]
        recs.append("@r%d\n%s\n+\n%s\n" % (i, "".join(rng.choice("ACGT") for _ in range(n)), qual))
    text = "".join(recs).encode()
    plain, gz = tmp_path / "p.fastq", tmp_path / "p.fastq.gz"
    plain.write_bytes(text)
    bgzf.write(gz, text, block_size=300)
    assert scan(lib, gz) == (0, -(-len(text) // 300) + 1, len(text))
    a, b = C.c_uint64(), C.c_uint64()
    for off in range(len(text) + 3):
        assert lib.bc_fastq_record_start(str(plain).encode(), off, C.byref(a)) == 0
        assert lib.bc_fastq_gz_record_start(str(gz).encode(), off, C.byref(b)) == 0
        assert a.value == b.value, off


def test_gz_record_start_refuses_a_plain_gzip_file(lib, tmp_path):
    import ngs_barcode_count_amd as pkg
    p = tmp_path / "g.fastq.gz"
    with gzip.open(p, "wb") as f:
        f.write(TEXT[:5000])
    v = C.c_uint64()
    assert lib.bc_fastq_gz_record_start(str(p).encode(), 100, C.byref(v)) == pkg._lib.BC_ERR_UNSUPPORTED
