"""`barcode-count -f reads.bam` against `-f reads.fastq` (the FASTQ text the BAM file means): the same files, the same
CSV contents, the same stdout and stats file once the clock lines and the input's name are masked -- on one rank and on
two."""
import os
import re
import subprocess

import pytest

import bam_cases
import cases
from test_gpu_bam_ingest import as_records
from test_gpu_cli import CLI, write_inputs

pytestmark = pytest.mark.gpu


def run_cli(tmp, reads, args, tag, extra=()):
    out = os.path.join(tmp, "out_" + tag)
    os.makedirs(out)
    res = subprocess.run([CLI, "-f", reads] + args + ["-o", out, "-p", "run", "-m", "-e"] + list(extra), capture_output=True, text=True,
                         env=dict(os.environ, BC_INGEST_CHUNK="65536"), timeout=600)
    assert res.returncode == 0, res.stderr + res.stdout
    mask = lambda text: text.replace(reads, "READS")
    stdout = re.sub(r"(Compute|Total) time: .*", r"\1 time: -", mask(res.stdout))
    lines = stdout.split("\n")  # (the progress counter rewrites its line once per chunk: of a run of totals the last one counts)
    stdout = "\n".join(line for i, line in enumerate(lines)
                       if not (line.startswith("Total sequences:") and lines[i + 1].startswith("Total sequences:")))
    produced = {}
    for fn in sorted(os.listdir(out)):
        data = open(os.path.join(out, fn), "rb").read()
        if fn.endswith("_barcode_stats.txt"):
            data = re.sub(rb"(Start|Finish|Compute time|Total time): .*", rb"\1: -", mask(data.decode()).encode())
        produced[fn] = data
    return stdout, produced


def test_cli_bam_equals_fastq(tmp_path):
    tmp = str(tmp_path)
    c = cases.build_case("del_mismatch_quality", seed=91, n=3000)
    args = write_inputs(tmp, dict(c, reads=c["reads"][:10]))[2:]  # (the scheme and CSV arguments; the reads follow)
    records = as_records(c["reads"], seed=11)
    bam, fq = os.path.join(tmp, "reads.bam"), os.path.join(tmp, "reads_text.fastq")
    bam_cases.write(bam, records, refs=((b"chr1", 1000),), block_size=20000, fastq_path=fq)
    out_fq, files_fq = run_cli(tmp, fq, args, "fastq")
    out_bam, files_bam = run_cli(tmp, bam, args, "bam")
    assert out_bam == out_fq
    assert "Total sequences:             {:,}".format(len(c["reads"])) in out_bam and "WARNING" not in out_bam and "gzip" not in out_bam
    assert sorted(files_bam) == sorted(files_fq) and len(files_bam) >= 3
    for fn in files_bam:
        assert files_bam[fn] == files_fq[fn], fn
    out_two, files_two = run_cli(tmp, bam, args, "bam_two_ranks", ["--gpus", "2", "--devices", "0,0", "--comm", "host"])
    assert "Total sequences:             {:,}".format(len(c["reads"])) in out_two
    assert sorted(files_two) == sorted(files_bam)
    for fn in files_two:
        if fn.endswith(".csv"):
            assert files_two[fn] == files_bam[fn], fn
