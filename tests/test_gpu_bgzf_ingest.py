"""Engine.count_fastq on BGZF files: the compressed bytes go to the device, one wavefront inflates one block, and the
counts are those of the same text read through zlib (a gzip.open file, the yardstick) and those of the oracle."""
import ctypes as C
import gzip
import os

import pytest

import bgzf
import cases
import parity

pytestmark = pytest.mark.gpu


def count_file(plan, path):
    import ngs_barcode_count_amd as pkg
    eng = pkg.Engine(plan, device=0)
    total = eng.count_fastq(path)
    got, rows, blocks = eng.counters(), eng.result_rows(), eng.gz_blocks_inflated()
    eng.close()
    return total, got, rows, blocks


def scan(path):
    import ngs_barcode_count_amd as pkg
    n, size = C.c_uint64(), C.c_uint64()
    assert pkg._lib.load().bc_bgzf_scan(str(path).encode(), C.byref(n), C.byref(size)) == 0
    return n.value


def write_three(tmp, stem, text, block_size):
    plain, single, blocked = (os.path.join(tmp, stem + ext) for ext in (".fastq", ".single.fastq.gz", ".bgzf.fastq.gz"))
    open(plain, "wb").write(text)
    with gzip.open(single, "wb") as f:
        f.write(text)
    bgzf.write(blocked, text, block_size=block_size)
    return plain, single, blocked


@pytest.mark.parametrize("chunk", [4096, None])
@pytest.mark.parametrize("block_size", [700, 65280])
@pytest.mark.parametrize("name", ["del_mismatch_quality", "fmtn"])  # fixed and ragged read lengths
def test_bgzf_counts_what_gzread_counts(tmp_path, monkeypatch, name, block_size, chunk):
    from test_gpu_parity import make_plan
    if chunk:
        monkeypatch.setenv("BC_INGEST_CHUNK", str(chunk))
    c = cases.build_case(name, seed=71, n=1500)
    text = "".join("@r%d %s\n%s\n+\n%s\n" % (i, "x" * (i % 37), s, q) for i, (s, q) in enumerate(c["reads"])).encode()
    plain, single, blocked = write_three(str(tmp_path), "reads", text, block_size)
    plan = make_plan(c)
    o = parity.oracle_for(c)
    for s, q in c["reads"]:
        o.process(s, q)
    t_plain, g_plain, r_plain, b_plain = count_file(plan, plain)
    t_single, g_single, r_single, b_single = count_file(plan, single)
    t_bgzf, g_bgzf, r_bgzf, b_bgzf = count_file(plan, blocked)
    assert (b_plain, b_single) == (0, 0) and b_bgzf == scan(blocked)
    assert (t_bgzf, g_bgzf, r_bgzf) == (t_single, g_single, r_single)
    assert t_bgzf == len(c["reads"]) + 1 and t_plain == len(c["reads"]) and (g_plain, r_plain) == (g_bgzf, r_bgzf)
    assert {k: g_bgzf[k] for k in o.counters} == o.counters and r_bgzf == o.rows()
    monkeypatch.setenv("BC_GZ_DEVICE", "0")
    assert count_file(plan, blocked) == (t_single, g_single, r_single, 0)


@pytest.mark.parametrize("block_size", [700, 65280])
def test_bgzf_end_of_stream_variants(tmp_path, block_size):
    """the gz quirks (test_gpu_cli.test_gz_without_a_final_newline): no final newline after line 4, after line 2, three
    lines into a record; and a quality line shorter than its sequence line"""
    from test_gpu_parity import make_plan
    c = cases.build_case("del_mismatch_quality", seed=61, n=500)
    plan = make_plan(c)
    reads = list(c["reads"])
    s_last, q_last = next((s, q) for s, q in reads if parity.oracle_for(c).process(s, q) == "matched")
    reads[-1] = (s_last, q_last)
    reads[7] = (reads[7][0], reads[7][1][:-9])  # a quality line shorter than its sequence line
    text = "".join("@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(reads))
    bodies = {"fourth_line": text[:-1], "second_line": text + "@tail\nACGTACGT", "third_line": text + "@tail\n" + s_last + "\n+\n",
              "third_line_open": text + "@tail\n" + s_last + "\n+", "whole": text}
    for variant, body in bodies.items():
        _, single, blocked = write_three(str(tmp_path), variant, body.encode(), block_size)
        want = count_file(plan, single)
        got = count_file(plan, blocked)
        assert got[:3] == want[:3], variant
        assert want[3] == 0 and got[3] == scan(blocked), variant
        assert got[0] == len(reads) + 1, (variant, got[0])
        o = parity.oracle_for(c)
        for i, (s, q) in enumerate(reads):
            o.process(s, q[:-1] if (variant == "fourth_line" and i == len(reads) - 1) else q)
        if variant.startswith("third_line"):
            o.process(s_last, "")
        assert {k: got[1][k] for k in o.counters} == o.counters and got[2] == o.rows(), variant


def test_a_flipped_payload_bit_is_a_read_error_and_the_engine_goes_on(tmp_path):
    import ngs_barcode_count_amd as pkg
    from test_gpu_parity import make_plan
    c = cases.build_case("del_mismatch_quality", seed=72, n=1500)
    text = "".join("@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(c["reads"])).encode()
    good = os.path.join(str(tmp_path), "good.fastq.gz")
    bgzf.write(good, text, block_size=20000)
    blob = bytearray(open(good, "rb").read())
    off, payload_off, payload_len, _, _ = bgzf.members(bytes(blob))[3]
    blob[payload_off + payload_len // 2] ^= 0x10
    bad = os.path.join(str(tmp_path), "bad.fastq.gz")
    open(bad, "wb").write(bytes(blob))
    assert scan(bad) == scan(good)  # the headers are untouched: still BGZF
    eng = pkg.Engine(make_plan(c), device=0)
    with pytest.raises(pkg.BarcodeCountError) as err:
        eng.count_fastq(bad)
    assert err.value.code == pkg._lib.BC_ERR_INVALID
    assert "read error in " + bad in str(err.value) and "file offset %d" % off in str(err.value)
    eng.reset()
    o = parity.oracle_for(c)
    for s, q in c["reads"]:
        o.process(s, q)
    assert eng.count_fastq(good) == len(c["reads"]) + 1
    got = eng.counters()
    assert {k: got[k] for k in o.counters} == o.counters and eng.result_rows() == o.rows()
    eng.close()
