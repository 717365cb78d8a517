"""bc_bam_scan, the host half of the BAM ingest (no GPU): the header's dictionary size and the inflated offset of the
first record, and the files it refuses."""
import os

import pytest

import bam_cases
import bgzf

TEXT = b"@HD\tVN:1.6\tSO:unsorted\n"
REFS = ((b"chr1", 1000), (b"a_longer_reference_name", 7), (b"x", 1 << 30))
RECORDS = [bam_cases.Rec(name=b"r%d" % i, seq="ACGT" * i, qual=[30] * (4 * i)) for i in range(5)]


def scan(path):
    import ngs_barcode_count_amd as pkg
    return pkg.bam_scan(path)


@pytest.mark.parametrize("name,text,refs,block_size", [("empty_dictionary", TEXT, (), 65280), ("three_references", TEXT, REFS, 65280),
                                                       ("text_over_many_blocks", TEXT + b"@CO\t" + b"c" * 3000 + b"\n", REFS, 100),
                                                       ("no_text", b"", (), 7)])
def test_scan_finds_the_first_record(tmp_path, name, text, refs, block_size):
    path = os.path.join(str(tmp_path), name + ".bam")
    at = bam_cases.write(path, RECORDS, text=text, refs=refs, block_size=block_size)
    head = bam_cases.header(text, refs)
    body, _ = bam_cases.records_text(RECORDS)
    assert scan(path) == (len(refs), len(head), len(head) + len(body)) and at[0] == len(head)


def test_a_header_only_file(tmp_path):
    path = os.path.join(str(tmp_path), "empty.bam")
    bam_cases.write(path, [], refs=REFS, eof_marker=False)
    n = len(bam_cases.header(TEXT, REFS))
    assert scan(path) == (3, n, n)


@pytest.mark.parametrize("name", ["bad_magic", "cut_in_the_text", "cut_in_the_dictionary", "cut_before_n_ref", "not_bgzf", "empty_file",
                                  "missing_file"])
def test_scan_refuses(tmp_path, name):
    import ngs_barcode_count_amd as pkg
    head = bam_cases.header(TEXT, REFS)
    path = os.path.join(str(tmp_path), name + ".bam")
    blob = {"bad_magic": b"BAM\2" + head[4:], "cut_in_the_text": head[:20], "cut_in_the_dictionary": head[:-6],
            "cut_before_n_ref": head[:8 + len(TEXT) + 2]}.get(name)
    if blob is not None:
        bgzf.write(path, blob, block_size=16)
    elif name == "not_bgzf":
        open(path, "wb").write(head)
    elif name == "empty_file":
        open(path, "wb").close()
    with pytest.raises(pkg.BarcodeCountError) as err:
        scan(path)
    assert err.value.code == pkg._lib.BC_ERR_INVALID
    want = {"bad_magic": "bad magic", "not_bgzf": "is not BGZF", "empty_file": "is not BGZF", "missing_file": "Failed to open file"}
    assert want.get(name, "runs past the end of the file") in str(err.value), str(err.value)


def test_the_two_exports_are_declared_and_bound():
    import ngs_barcode_count_amd as pkg
    import test_abi_symbols
    names = test_abi_symbols.declared_functions()
    assert {"bc_bam_scan", "bc_bam_frame_device"} <= set(names) & set(pkg._lib.ENGINE_API)
    test_abi_symbols.test_library_exports_every_declared_symbol()
