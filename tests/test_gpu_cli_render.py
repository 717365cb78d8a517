"""`barcode-count` on dense plans, whose full-counts files now come from the device as text (bc_engine_render_counts /
bc_engine_render_merged) instead of per-row host strings: every file against the reference's writers
(tests/pyref_output.py) over the oracle's counts, the device path against the host path (BC_DEVICE_WRITERS=0), and the
order of the lines, which is ascending dense index on the device path and the same on every run."""
import os
import re
import subprocess

import pytest

import cases
import pyref_output  # noqa: F401  (the writers `expected` runs)
from test_gpu_cli import CLI, canonical, expected, read_csv, write_inputs

pytestmark = pytest.mark.gpu

DEVICE = "[barcode-count] writers: device text (bc_engine_render_counts)"
HOST = "[barcode-count] writers: per-row strings"
CLOCK = re.compile(r"^(Start|Finish|Total time|Compute time).*$", re.M)


def run_cli(tmp, args, tag, merge, enrich, extra=(), env=None):
    out = os.path.join(tmp, tag)
    os.makedirs(out)
    cmd = [CLI] + args + ["-o", out, "-p", "r"] + (["-m"] if merge else []) + (["-e"] if enrich else []) + list(extra)
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, BC_WRITERS_VERBOSE="1", BC_ENRICH_VERBOSE="1", **(env or {})))
    assert res.returncode == 0, res.stderr + res.stdout
    return out, res


def compare_with_reference(out, c, merge, enrich):
    o, w = expected(c, "r", merge, enrich)
    produced = sorted(f for f in os.listdir(out) if f.endswith(".csv"))
    assert produced == sorted(w.files), (produced, sorted(w.files))
    for fn, (header, rows) in w.files.items():
        h, r = read_csv(os.path.join(out, fn))
        if ".all." in fn:
            assert canonical(h, r, o.barcode_num) == canonical(header, rows, o.barcode_num), fn
        else:
            assert (h, r) == (header, rows), fn
    stats = open(os.path.join(out, "r_barcode_stats.txt")).read()
    listed = re.findall(r"File & barcodes counted: (\S+)\t([\d,]+)", stats)
    if c.get("samples"):
        assert [f for f, _ in listed] == w.output_files
        assert [int(n.replace(",", "")) for _, n in listed] == w.output_counts
    else:
        assert sorted(listed) == sorted(zip(w.output_files, ["{:,}".format(n) for n in w.output_counts]))
    return o, w


def full_counts_files(out):
    return sorted(f for f in os.listdir(out) if f.endswith(".csv") and ".Single." not in f and ".Double." not in f)


def dense_index_of(line, c):
    """the dense tuple index of a counts line (IDs are bb<g>_<sequence>, write_inputs)"""
    parts = line.split(",")
    t = 0
    for g, refs in enumerate(c["counted"]):
        assert parts[g].startswith("bb%d_" % (g + 1))
        t = t * len(refs) + refs.index(parts[g][len("bb%d_" % (g + 1)):])
    return t


def device_vs_host(tmp_path, c, merge, enrich, extra=(), expect_device=True):
    tmp = str(tmp_path)
    args = write_inputs(tmp, c)
    out_d, res_d = run_cli(tmp, args, "dev", merge, enrich, extra)
    assert (DEVICE if expect_device else HOST) in res_d.stderr, res_d.stderr[-600:]
    compare_with_reference(out_d, c, merge, enrich)
    out_h, res_h = run_cli(tmp, args, "host", merge, enrich, extra, env={"BC_DEVICE_WRITERS": "0"})
    assert HOST in res_h.stderr, res_h.stderr[-600:]
    # the same file set, headers and sorted lines; the same stdout and stats file up to the clock lines
    assert sorted(os.listdir(out_d)) == sorted(os.listdir(out_h))
    for f in os.listdir(out_d):
        if f.endswith(".csv"):
            assert read_csv(os.path.join(out_d, f)) == read_csv(os.path.join(out_h, f)), f
    mask = lambda text, out: CLOCK.sub("", text.replace(out, "<out>"))
    assert mask(res_d.stdout, out_d) == mask(res_h.stdout, out_h)
    stats = [mask(open(os.path.join(o, "r_barcode_stats.txt")).read(), o) for o in (out_d, out_h)]
    assert stats[0] == stats[1]
    if not expect_device:
        return out_d
    # a second device-path run: the full-counts files byte for byte, their lines in ascending index order
    out_2, res_2 = run_cli(tmp, args, "dev2", merge, enrich, extra)
    assert DEVICE in res_2.stderr
    files = full_counts_files(out_d)
    assert files
    for f in files:
        data = open(os.path.join(out_d, f), "rb").read()
        assert data == open(os.path.join(out_2, f), "rb").read(), f
        idx = [dense_index_of(line, c) for line in data.decode().split("\n")[1:-1]]
        assert idx == sorted(idx) and len(set(idx)) == len(idx), f
    return out_d


@pytest.mark.parametrize("merge,enrich", [(False, False), (True, False), (False, True), (True, True)])
def test_del(tmp_path, merge, enrich):
    c = cases.build_case("del_mismatch_quality", seed=61, n=3000)
    device_vs_host(tmp_path, c, merge, enrich)


def test_crispr_without_sample_group(tmp_path):
    c = cases.build_case("crispr", seed=62, n=3000)
    out = device_vs_host(tmp_path, c, True, False)  # (-m with one key: "Merged file cannot be created", both paths)
    assert full_counts_files(out) == ["r_barcode_counts.csv"]


@pytest.mark.parametrize("merge", [False, True])
def test_random_barcode(tmp_path, merge):
    c = cases.build_case("del_random", seed=63, n=3000)
    device_vs_host(tmp_path, c, merge, False)


def test_sample_without_reads(tmp_path):
    c = cases.build_case("del_mismatch_quality", seed=64, n=2000)
    c["samples"] = dict(c["samples"], TTTTTTTT="Z_no_reads")
    out = device_vs_host(tmp_path, c, True, True)
    assert open(os.path.join(out, "r_Z_no_reads_counts.csv")).read() == "Barcode_1,Barcode_2,Barcode_3,Count\n"


def test_several_ranks(tmp_path):
    c = cases.build_case("del_mismatch_quality", seed=65, n=3001)
    device_vs_host(tmp_path, c, True, False, ["--gpus", "2", "--devices", "0,0", "--comm", "host"])


@pytest.mark.parametrize("name,merge,enrich", [("example_files_random_nosample", True, True),
                                               ("nosample_with_sample_file", False, False)])
def test_sample_file_without_sample_group_keeps_the_rows(tmp_path, name, merge, enrich):
    """the "barcode" key of these runs exists only once a row lands on it (info.rs:792-801): the writers need the rows
    to know, so the run stays on the host path, and writes what the reference writes"""
    c = cases.build_case(name, seed=66, n=2500)
    device_vs_host(tmp_path, c, merge, enrich, expect_device=False)


@pytest.mark.parametrize("enrich", [False, True])
def test_raw_keys_report_the_host_path(tmp_path, enrich):
    """plans whose keys are raw captures have no index form.  (The other guard of the device path, an ID with a comma
    under -e, cannot be reached from the command line: the counted-barcode file is split at every comma, so no ID it
    loads holds one.)"""
    c = cases.build_case("raw_counted", seed=67, n=1500)
    device_vs_host(tmp_path, c, False, enrich, expect_device=False)


def test_progress_lines_of_a_file_above_50_000_rows(tmp_path):
    """add_counts_string prints `Barcodes counted: N\\r` every 50,000 rows; the device path prints the same bytes from the
    row count.  300,000 synthetic reads over 2 x 48^3 tuples leave more than 50,000 rows in each sample's file."""
    import workloads
    w = workloads.make("config3", n_sets=(2, 48, 48, 48))
    n, R = 300_000, w.read_len
    seq, qual = w.synth.generate_host(0, n)
    seq, qual = seq.reshape(n, R), qual.reshape(n, R)
    tmp = str(tmp_path)
    fq = os.path.join(tmp, "reads.fastq")
    with open(fq, "wb") as f:
        for i in range(n):
            f.write(b"@r%d\n" % i + seq[i].tobytes() + b"\n+\n" + qual[i].tobytes() + b"\n")
    open(os.path.join(tmp, "scheme.txt"), "w").write(w.scheme + "\n")
    open(os.path.join(tmp, "samples.csv"), "w").write(
        "Barcode,Sample_ID\n" + "".join("%s,sample_%d\n" % (s, i) for i, s in enumerate(w.samples)))
    open(os.path.join(tmp, "counted.csv"), "w").write("Barcode,Barcode_ID,Barcode_Number\n" + "".join(
        "%s,bb%d_%d,%d\n" % (s, b + 1, i, b + 1) for b, refs in enumerate(w.counted) for i, s in enumerate(refs)))
    args = ["-f", fq, "-q", os.path.join(tmp, "scheme.txt"), "-s", os.path.join(tmp, "samples.csv"), "-c",
            os.path.join(tmp, "counted.csv"), "--min-quality", "20"]
    out_d, res_d = run_cli(tmp, args, "dev", True, False)
    out_h, res_h = run_cli(tmp, args, "host", True, False, env={"BC_DEVICE_WRITERS": "0"})
    assert DEVICE in res_d.stderr and HOST in res_h.stderr
    # (once per sample file; the pipe is read in text mode, which hands the carriage return over as a newline)
    assert len(re.findall(r"Barcodes counted: 50,000[\r\n]", res_d.stdout)) == 2, res_d.stdout[-600:]
    assert CLOCK.sub("", res_d.stdout) == CLOCK.sub("", res_h.stdout)
    for f in os.listdir(out_d):
        if f.endswith(".csv"):
            assert read_csv(os.path.join(out_d, f)) == read_csv(os.path.join(out_h, f)), f
            assert len(read_csv(os.path.join(out_d, f))[1]) > 50_000, f
