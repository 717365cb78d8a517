"""Engine.count_fastq on unaligned BAM files: the BGZF blocks are inflated and the records framed on the device, and
the counts are those of the plain FASTQ file the BAM file means (bam_cases.py works that text out in plain Python) and
those of the oracle over the same text."""
import os
import random

import pytest

import bam_cases
import cases
import parity
from bam_cases import Rec

pytestmark = pytest.mark.gpu

LONG = "long_match_kernel"


def as_records(reads, seed, extras=True):
    """BAM records that mean `reads` [(sequence line, quality line)]: every third one stored reverse-complemented with
    the reverse flag, names, CIGARs and aux fields of many lengths, and secondary and supplementary records in between"""
    rng = random.Random(seed)
    out = []
    for i, (s, q) in enumerate(reads):
        flag = rng.choice([4, 77, 141, 0])
        qual = [ord(ch) - 33 for ch in q]
        if i % 3 == 1:
            flag |= 0x10
            s, qual = "".join(bam_cases.COMPLEMENT[ch] for ch in reversed(s)), qual[::-1]
        aux = rng.choice([b"", b"RGZgroup1\0", b"XBBC" + bytes([5, 0, 0, 0, 1, 2, 3, 4, 5]), b"MMZ" + b"C+m," * rng.randrange(1, 30) + b"\0"])
        out.append(Rec(name=b"read/%d" % i + b"x" * (i % 41), flag=flag, seq=s, qual=qual, cigar=[len(s) << 4] * (i % 3), aux=aux))
        if extras and i % 50 == 7:
            out.append(Rec(name=b"sec", flag=rng.choice([0x100, 0x800, 0x910]), seq=s[:20], qual=qual[:20]))
    return out


def oracle_over(c, records):
    o = parity.oracle_for(c)
    reads = [r.fastq() for r in records]
    for sq in reads:
        if sq is not None:
            o.process(*sq)
    return o, sum(sq is not None for sq in reads)


def check_engine(eng, o, n_reads):
    got = eng.counters()
    assert {k: got[k] for k in o.counters} == o.counters and eng.result_rows() == o.rows()
    assert got["total_reads"] == n_reads


@pytest.mark.parametrize("chunk,block_size", [(4096, 700), (None, 65280)])
@pytest.mark.parametrize("name", ["del_exact", "del_mismatch_quality", "raw_counted"])
def test_bam_counts_what_its_fastq_counts(tmp_path, monkeypatch, name, chunk, block_size):
    import ngs_barcode_count_amd as pkg
    from test_gpu_parity import make_plan
    if chunk:
        monkeypatch.setenv("BC_INGEST_CHUNK", str(chunk))
    c = cases.build_case(name, seed=81, n=2500)
    records = as_records(c["reads"], seed=5)
    bam, fq = os.path.join(str(tmp_path), "reads.bam"), os.path.join(str(tmp_path), "reads.fastq")
    bam_cases.write(bam, records, refs=((b"chr1", 1000), (b"chr2", 5)), block_size=block_size, fastq_path=fq)
    o, n_reads = oracle_over(c, records)
    assert n_reads == len(c["reads"]) and len(records) > n_reads
    eng = pkg.Engine(make_plan(c), device=0)
    assert eng.count_fastq(bam) == n_reads
    from_bam = (eng.counters(), eng.result_rows())
    check_engine(eng, o, n_reads)
    assert eng.gz_blocks_inflated() > 0
    eng.reset_results()  # (a fresh table; the outcome counters go on)
    assert eng.count_fastq(fq) == n_reads
    assert (eng.counters(), eng.result_rows()) == ({k: 2 * v for k, v in from_bam[0].items()}, from_bam[1])
    eng.close()


def test_reverse_secondary_supplementary_and_missing_qualities(tmp_path):
    import ngs_barcode_count_amd as pkg
    from test_gpu_parity import make_plan
    c = cases.build_case("del_mismatch_quality", seed=82, n=2000)
    records = as_records(c["reads"], seed=6)
    for i in range(0, len(records), 4):  # a quarter of the records store no qualities: every base gets Phred 1
        records[i].qual = None
    for i in range(1, len(records), 9):  # IUPAC letters pass through as themselves, complemented on the reverse strand
        records[i].seq = records[i].seq[:3] + "RYKM" + records[i].seq[7:]
    for i in range(2, len(records), 11):
        records[i].qual = [min(255, q + 200) for q in records[i].qual] if records[i].qual else None  # above 93: clamped
    bam = os.path.join(str(tmp_path), "mixed.bam")
    bam_cases.write(bam, records, block_size=3000)
    o, n_reads = oracle_over(c, records)
    eng = pkg.Engine(make_plan(c), device=0)
    assert eng.count_fastq(bam) == n_reads
    check_engine(eng, o, n_reads)
    assert o.counters["low_quality"] > 100 and o.counters["matched"] > 100
    eng.close()


def test_reads_of_330_bases_take_the_wave_per_read_kernel(tmp_path, monkeypatch):
    import ngs_barcode_count_amd as pkg
    from test_gpu_parity import make_plan
    monkeypatch.setenv("BC_INGEST_CHUNK", "4096")
    c = cases.build_case("del_exact", seed=83, n=2000)
    rng = random.Random(9)
    reads = [(s + "".join(rng.choice("ACGT") for _ in range(330 - len(s))), q + "I" * (330 - len(q))) for s, q in c["reads"]]
    reads[5] = (reads[5][0][:17], reads[5][1][:17])
    reads[6] = ("", "")
    records = as_records(reads, seed=7)
    bam = os.path.join(str(tmp_path), "long.bam")
    bam_cases.write(bam, records, block_size=700)
    o, n_reads = oracle_over(c, records)
    eng = pkg.Engine(make_plan(c), device=0)
    assert eng.count_fastq(bam) == n_reads
    assert eng.kernel_name() == LONG
    check_engine(eng, o, n_reads)
    eng.close()


def test_header_only_files_and_a_missing_eof_marker(tmp_path):
    import ngs_barcode_count_amd as pkg
    from test_gpu_parity import make_plan
    c = cases.build_case("del_exact", seed=84, n=2000)
    eng = pkg.Engine(make_plan(c), device=0)
    for eof_marker in (True, False):
        for block_size in (65280, 10):
            empty = os.path.join(str(tmp_path), "empty_%d_%d.bam" % (eof_marker, block_size))
            bam_cases.write(empty, [], refs=((b"chr1", 1000),), eof_marker=eof_marker, block_size=block_size)
            assert eng.count_fastq(empty) == 0
    assert eng.counters()["total_reads"] == 0
    records = as_records(c["reads"], seed=8)
    bam = os.path.join(str(tmp_path), "no_eof.bam")
    bam_cases.write(bam, records, eof_marker=False, block_size=5000)
    o, n_reads = oracle_over(c, records)
    assert eng.count_fastq(bam) == n_reads
    check_engine(eng, o, n_reads)
    eng.close()


def test_damaged_files_are_refused_and_the_engine_goes_on(tmp_path, monkeypatch):
    import ngs_barcode_count_amd as pkg
    from test_gpu_parity import make_plan
    c = cases.build_case("del_exact", seed=85, n=2000)
    records = as_records(c["reads"], seed=9)
    good = os.path.join(str(tmp_path), "good.bam")
    at = bam_cases.write(good, records, block_size=5000)
    head = bam_cases.header()
    body, _ = bam_cases.records_text(records)
    assert at[0] == len(head)
    damaged = {
        "cut_mid_record": (head + body[:at[1500] - at[0] + 50], pkg._lib.BC_ERR_INVALID, "ends inside a BAM record"),
        "cut_mid_header": (head + body[:at[1500] - at[0] + 20], pkg._lib.BC_ERR_INVALID, "ends inside a BAM record"),
        "block_size_off_by_one": (head + body[:at[700] - at[0]] + bytes([body[at[700] - at[0]] + 1]) + body[at[700] - at[0] + 1:],
                                  pkg._lib.BC_ERR_INVALID, "the chain of BAM records breaks"),
        "bad_magic": (b"BAM\2" + head[4:] + body, pkg._lib.BC_ERR_INVALID, "bad magic"),
        "l_seq_70000": (head + body[:at[900] - at[0]] + Rec(seq="ACGT" * 17500, qual=[30] * 70000).pack() + body[at[900] - at[0]:],
                        pkg._lib.BC_ERR_UNSUPPORTED, "a FASTQ line is longer than 65535 bytes (not supported by the engine)"),
        "record_of_5_mib": (head + body[:at[900] - at[0]] + Rec(seq="AC", aux=b"XZZ" + b"." * (5 << 20) + b"\0").pack() + body[at[900] - at[0]:],
                            pkg._lib.BC_ERR_UNSUPPORTED, "is longer than 4 MiB"),
    }
    eng = pkg.Engine(make_plan(c), device=0)
    o, n_reads = oracle_over(c, records)
    for name, (blob, code, words) in damaged.items():
        path = os.path.join(str(tmp_path), name + ".bam")
        import bgzf
        bgzf.write(path, blob, block_size=5000 if len(blob) < (1 << 20) else 65280)
        with pytest.raises(pkg.BarcodeCountError) as err:
            eng.count_fastq(path)
        assert err.value.code == code and words in str(err.value), (name, str(err.value))
    not_bgzf = os.path.join(str(tmp_path), "plain.bam")
    open(not_bgzf, "wb").write(head + body)
    with pytest.raises(pkg.BarcodeCountError) as err:
        eng.count_fastq(not_bgzf)
    assert err.value.code == pkg._lib.BC_ERR_INVALID and "is not BGZF" in str(err.value)
    blob = bytearray(open(good, "rb").read())
    import bgzf
    off, payload_off, payload_len, _, _ = bgzf.members(bytes(blob))[3]
    blob[payload_off + payload_len // 2] ^= 0x10
    flipped = os.path.join(str(tmp_path), "flipped.bam")
    open(flipped, "wb").write(bytes(blob))
    with pytest.raises(pkg.BarcodeCountError) as err:
        eng.count_fastq(flipped)
    assert err.value.code == pkg._lib.BC_ERR_INVALID and "BGZF block at file offset %d" % off in str(err.value)
    eng.reset()
    assert eng.count_fastq(good) == n_reads
    check_engine(eng, o, n_reads)
    eng.close()


def test_two_shards_and_the_verbose_line(tmp_path, monkeypatch, capfd):
    import ngs_barcode_count_amd as pkg
    from test_gpu_parity import make_plan
    monkeypatch.setenv("BC_INGEST_VERBOSE", "1")
    monkeypatch.setenv("BC_GZ_DEVICE", "0")  # (about .gz names: a .bam goes the device way all the same)
    c = cases.build_case("del_exact", seed=86, n=2000)
    records = as_records(c["reads"], seed=10)
    bam = os.path.join(str(tmp_path), "reads.bam")
    bam_cases.write(bam, records, block_size=5000)
    o, n_reads = oracle_over(c, records)
    eng = pkg.Engine(make_plan(c), device=0)
    assert eng.count_fastq(bam, shard=1, n_shards=2) == 0 and eng.counters()["total_reads"] == 0
    assert eng.count_fastq(bam, shard=0, n_shards=2) == n_reads
    check_engine(eng, o, n_reads)
    eng.close()
    err = capfd.readouterr().err
    assert err.count("path bam-device") == 2 and "shard 0/2" in err and "%d records counted" % n_reads in err
