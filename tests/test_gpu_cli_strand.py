"""`barcode-count --strand both` on a mixed-orientation FASTQ file and on the same reads as unaligned BAM (flag 4, no
0x10 anywhere) against a plain run on the FASTQ file oriented on the host -- the input the oracle composition defines;
and `--strand forward` against no flag at all."""
import os
import re

import pytest

import bam_cases
import cases
import strand_cases as sc
from test_gpu_cli import write_inputs
from test_gpu_cli_bam import run_cli

pytestmark = pytest.mark.gpu

COUNTER_LINES = ("Total sequences:", "Correctly matched sequences:", "Constant region mismatches:", "Sample barcode mismatches:",
                 "Counted barcode mismatches:", "Duplicates:", "Low quality barcodes:")
EXTRA = "Reverse strand matches:"


def write_fastq(path, reads):
    with open(path, "w") as f:
        f.write("".join("@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(reads)))


def counter_lines(stdout):
    """the last line of each counter (the progress line rewrites "Total sequences:")"""
    out = {}
    for line in stdout.replace("\r", "\n").split("\n"):
        for k in COUNTER_LINES + (EXTRA,):
            if line.startswith(k):
                out[k] = line[len(k):].strip()
    return out


def csv_lines(files):
    return {fn: sorted(data.split(b"\n")) for fn, data in files.items() if fn.endswith(".csv")}


def test_cli_both_equals_the_host_oriented_run(tmp_path):
    tmp = str(tmp_path)
    c = sc.mix(cases.build_case("del_mismatch_quality", seed=93, n=2000), 93)
    exp = sc.expected(c, "both")
    assert exp["matched_reverse"] > 400 and exp["counters"]["matched"] > exp["matched_reverse"] + 400
    args = write_inputs(tmp, dict(c, reads=c["reads"][:10]))[2:]  # (the scheme and CSV arguments; the reads follow)
    mixed, oriented, bam = (os.path.join(tmp, n) for n in ("mixed.fastq", "oriented.fastq", "mixed.bam"))
    write_fastq(mixed, c["reads"])
    write_fastq(oriented, exp["reads"])
    bam_cases.write(bam, [bam_cases.Rec(name=b"r%d" % i, flag=4, seq=s, qual=[ord(ch) - 33 for ch in q]) for i, (s, q) in enumerate(c["reads"])],
                    block_size=20000)
    out_ref, files_ref = run_cli(tmp, oriented, args, "oriented")
    ref = counter_lines(out_ref)
    assert EXTRA not in ref and ref["Correctly matched sequences:"] == "{:,}".format(exp["counters"]["matched"])
    for tag, path in (("fastq", mixed), ("bam", bam)):
        out, files = run_cli(tmp, path, args, "both_" + tag, ["--strand", "both"])
        got = counter_lines(out)
        assert got.pop(EXTRA) == "{:,}".format(exp["matched_reverse"]), tag
        assert got == ref, tag
        assert sorted(files) == sorted(files_ref) and len(files) >= 3
        assert csv_lines(files) == csv_lines(files_ref), tag
        stats = [fn for fn in files if fn.endswith("_barcode_stats.txt")][0]
        assert (EXTRA + "      {:,}\n".format(exp["matched_reverse"])).encode() in files[stats]
        # the line follows the six counters, on stdout and in the stats file
        assert re.search(r"Low quality barcodes: +[\d,]+\n" + EXTRA, out) and re.search(rb"Low quality barcodes: +[\d,]+\n" + EXTRA.encode(), files[stats])
    # forward on the mixed file: its reverse half is lost to the constant region, which is what the option is for
    out_fwd, files_fwd = run_cli(tmp, mixed, args, "forward", ["--strand", "forward"])
    out_none, files_none = run_cli(tmp, mixed, args, "none")
    assert out_fwd == out_none and EXTRA not in out_fwd
    assert sorted(files_fwd) == sorted(files_none)
    for fn in files_fwd:
        if fn.endswith(".csv"):  # (row order within a file is the compaction's)
            assert sorted(files_fwd[fn].split(b"\n")) == sorted(files_none[fn].split(b"\n")), fn
        else:
            assert files_fwd[fn] == files_none[fn], fn
    assert int(counter_lines(out_fwd)["Constant region mismatches:"].replace(",", "")) > exp["retried"] * 9 // 10


def test_cli_reverse_and_refusal(tmp_path):
    import subprocess
    from test_gpu_cli import CLI
    tmp = str(tmp_path)
    c = cases.build_case("crispr", seed=94, n=800)
    exp = sc.expected(c, "forward")
    args = write_inputs(tmp, dict(c, reads=c["reads"][:10]))[2:]
    flipped = os.path.join(tmp, "flipped.fastq")
    write_fastq(flipped, [sc.rc(s, q) for s, q in c["reads"]])
    out, _ = run_cli(tmp, flipped, args, "reverse", ["--strand=reverse"])
    got = counter_lines(out)
    assert got[EXTRA] == got["Correctly matched sequences:"] == "{:,}".format(exp["counters"]["matched"])
    res = subprocess.run([CLI, "-f", flipped] + args + ["--strand", "sideways"], capture_output=True, text=True, timeout=60)
    assert res.returncode != 0 and "--strand must be forward, reverse or both" in res.stderr + res.stdout
