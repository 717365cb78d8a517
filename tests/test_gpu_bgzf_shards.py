"""Shards of a BGZF file (bc_fastq_count_shard, barcode-count --gpus N): every rank inflates only the blocks that cover
its share of the records, and the shards add up to what one call counts."""
import ctypes as C
import os
import subprocess

import pytest

import bgzf
import cases
from test_gpu_cli import CLI, canonical, expected, read_csv, write_inputs

pytestmark = pytest.mark.gpu


def scan(path):
    import ngs_barcode_count_amd as pkg
    n, size = C.c_uint64(), C.c_uint64()
    assert pkg._lib.load().bc_bgzf_scan(str(path).encode(), C.byref(n), C.byref(size)) == 0
    return n.value, size.value


def shard_runs(plan, fq, n_shards):
    import ngs_barcode_count_amd as pkg
    engs = [pkg.Engine(plan, device=0) for _ in range(n_shards)]
    totals = [e.count_fastq(fq, shard=k, n_shards=n_shards) for k, e in enumerate(engs)]
    counters = [e.counters() for e in engs]
    rows = {}
    for e in engs:
        for r in e.result_rows():
            rows[tuple(r[:-1])] = rows.get(tuple(r[:-1]), 0) + r[-1]
    blocks = [e.gz_blocks_inflated() for e in engs]
    for e in engs:
        e.close()
    summed = {k: sum(c[k] for c in counters) for k in counters[0]}
    return totals, summed, rows, blocks, counters


@pytest.mark.parametrize("block_size,n_reads", [(700, 1200), (65280, 1200), (700, 3)])
def test_bgzf_shards_add_up_to_the_single_call(tmp_path, monkeypatch, block_size, n_reads):
    import ngs_barcode_count_amd as pkg
    from test_gpu_parity import make_plan
    monkeypatch.setenv("BC_INGEST_CHUNK", "32768")
    c = cases.build_case("del_mismatch_quality", seed=43, n=n_reads)
    c["reads"] = [(s, ("@" + q[1:]) if i % 2 == 0 else q) for i, (s, q) in enumerate(c["reads"])]
    text = "".join("@read_%d some description\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(c["reads"])).encode()
    fq = os.path.join(str(tmp_path), "reads.fastq.gz")
    bgzf.write(fq, text, block_size=block_size)
    n_blocks, _ = scan(fq)
    plan = make_plan(c)
    whole = pkg.Engine(plan, device=0)
    total = whole.count_fastq(fq)
    assert total == len(c["reads"]) + 1 and whole.gz_blocks_inflated() == n_blocks
    ref_counters = whole.counters()
    ref_rows = {tuple(r[:-1]): r[-1] for r in whole.result_rows()}
    whole.close()
    for n in (2, 3, 5):  # (5 shards of 3 reads: fewer records than shards; the last boundary falls on the last record)
        totals, summed, rows, blocks, counters = shard_runs(plan, fq, n)
        print(n, totals, blocks)
        assert sum(totals) == total, totals
        assert summed == ref_counters and rows == ref_rows
        assert all(b > 0 for b, cn in zip(blocks, counters) if cn["total_reads"] > 0), blocks
        assert sum(blocks) <= n_blocks + 2 * (n - 1), (blocks, n_blocks)


@pytest.mark.parametrize("gpus,comm", [(2, "host"), (3, "host")])
def test_cli_on_several_ranks_reads_a_bgzf_file(tmp_path, gpus, comm):
    """the pattern of test_gpu_cli.test_cli_on_several_ranks_writes_what_one_rank_writes, on a BGZF input: every rank
    is on the bgzf-device path and the files are those one rank writes (all ranks on device 0, as there: ranks that
    share a device exchange through message files, RCCL wants a device per rank)"""
    c = cases.build_case("del_mismatch_quality", seed=41, n=3001)
    c["reads"] = [(s, ("@" + q[1:]) if q and i % 3 == 0 else q) for i, (s, q) in enumerate(c["reads"])]
    tmp = str(tmp_path)
    args = write_inputs(tmp, c)
    plain = args[1]
    fq = plain + ".gz"
    bgzf.write(fq, open(plain, "rb").read(), block_size=9000)
    args[1] = fq
    out = os.path.join(tmp, "out")
    os.makedirs(out)
    cmd = [CLI] + args + ["-o", out, "-p", "multi", "-m", "--gpus", str(gpus), "--devices", ",".join(["0"] * gpus)]
    if comm:
        cmd += ["--comm", comm]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, BC_INGEST_CHUNK="65536", BC_INGEST_VERBOSE="1"))
    assert res.returncode == 0, res.stderr + res.stdout
    o, w = expected(c, "multi", True, False)
    produced = sorted(f for f in os.listdir(out) if f.endswith(".csv"))
    assert produced == sorted(w.files), (produced, sorted(w.files))
    for fn, (header, rows) in w.files.items():
        h, r = read_csv(os.path.join(out, fn))
        if ".all." in fn:
            assert canonical(h, r, o.barcode_num) == canonical(header, rows, o.barcode_num), fn
        else:
            assert (h, r) == (header, rows), fn
    assert ("Total sequences:             {:,}".format(len(c["reads"]) + 1)) in res.stdout
    for label, key in (("Correctly matched sequences: ", "matched"), ("Constant region mismatches:  ", "constant_region"),
                       ("Low quality barcodes:        ", "low_quality")):
        assert label + "{:,}".format(o.counters[key]) in res.stdout, label
    said = [l for l in res.stderr.splitlines() if l.startswith("[bc ingest]")]
    assert len(said) == gpus and all("path bgzf-device" in l for l in said), res.stderr
    assert sorted(int(l.split("shard ")[1].split("/")[0]) for l in said) == list(range(gpus))
