"""`barcode-count -e` on dense plans, whose Single / Double maps now come from the device (bc_engine_enrich) instead of
six string-map insertions per row: every file against the reference's writers (tests/pyref_output.py) over the
oracle's counts, as test_gpu_cli.test_cli_outputs compares them -- with IDs shared inside a group, four counted
barcodes, a random barcode, a sample that receives no read, and several ranks."""
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import parity
import pyref_output
import readgen
from test_gpu_cli import CLI, canonical, expected, read_csv
from test_gpu_cli import write_inputs as write_plain_inputs

pytestmark = pytest.mark.gpu

DEL4_SCHEME = "[8]AGCTACGAATCG{8}TGGA{8}TGGA{8}TGGA{7}ACTAGAT"


def write_inputs(tmp, c, ids):
    """FASTQ, scheme, sample file and a counted-barcode file whose IDs come from ids[b][seq]"""
    fq = os.path.join(tmp, "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(c["reads"])))
    scheme = os.path.join(tmp, "scheme.txt")
    open(scheme, "w").write(c["scheme"] + "\n")
    sp = os.path.join(tmp, "samples.csv")
    open(sp, "w").write("Barcode,Sample_ID\n" + "".join("%s,%s\n" % kv for kv in c["samples"].items()))
    cp = os.path.join(tmp, "counted.csv")
    open(cp, "w").write("Barcode,Barcode_ID,Barcode_Number\n" + "".join(
        "%s,%s,%d\n" % (s, ids[b][s], b + 1) for b, refs in enumerate(c["counted"]) for s in refs))
    args = ["-f", fq, "-q", scheme, "-s", sp, "-c", cp]
    kw = c.get("kwargs", {})
    for flag, key in (("--max-errors-sample", "max_sample"), ("--max-errors-counted-barcode", "max_barcode"),
                      ("--max-errors-constant", "max_constant"), ("--min-quality", "min_quality")):
        if kw.get(key) is not None:
            args += [flag, str(kw[key])]
    return args


def run_and_compare(tmp_path, c, ids, merge, extra=()):
    tmp = str(tmp_path)
    args = write_inputs(tmp, c, ids)
    out = os.path.join(tmp, "out")
    os.makedirs(out)
    cmd = [CLI] + args + ["-o", out, "-p", "enr", "-e"] + (["-m"] if merge else []) + list(extra)
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, BC_ENRICH_VERBOSE="1"))
    assert res.returncode == 0, res.stderr + res.stdout
    assert "[barcode-count] enrichment: device marginal sums" in res.stderr, res.stderr[-500:]
    o = parity.oracle_for(c)
    for s, q in c["reads"]:
        o.process(s, q)
    results = {k: {} for k in o.sample_keys()}
    for s, t, n in o.rows():
        results.setdefault(s, {})[t] = n
    w = pyref_output.Writer(results, dict(c["samples"]), ids, o.barcode_num, "enr", merge, True).write()
    produced = sorted(f for f in os.listdir(out) if f.endswith(".csv"))
    assert produced == sorted(w.files), (produced, sorted(w.files))
    for fn, (header, rows) in w.files.items():
        h, r = read_csv(os.path.join(out, fn))
        if ".all." in fn:
            assert canonical(h, r, o.barcode_num) == canonical(header, rows, o.barcode_num), fn
        else:
            assert (h, r) == (header, rows), fn
    # the stats file lists the files and their row counts in the writers' order
    stats = open(os.path.join(out, "enr_barcode_stats.txt")).read()
    listed = re.findall(r"File & barcodes counted: (\S+)\t([\d,]+)", stats)
    assert [f for f, _ in listed] == w.output_files
    assert [int(n.replace(",", "")) for _, n in listed] == w.output_counts
    for fn in w.output_files:
        assert fn in res.stdout
    return w


def unique_ids(c):
    return [{s: "bb%d_%s" % (b + 1, s) for s in refs} for b, refs in enumerate(c["counted"])]


@pytest.mark.parametrize("merge", [False, True])
def test_del_with_ids_shared_inside_a_group(tmp_path, merge):
    c = cases.build_case("del_mismatch_quality", seed=51, n=3000)
    # every two sequences of a group share an ID (their enrichment counts add up), one ID is empty
    ids = [{s: "B%d_%d" % (b + 1, i // 2) for i, s in enumerate(refs)} for b, refs in enumerate(c["counted"])]
    ids[1][c["counted"][1][5]] = ""
    w = run_and_compare(tmp_path, c, ids, merge)
    assert any(".Double." in f for f in w.files) and any(".Single." in f for f in w.files)


@pytest.mark.parametrize("merge", [False, True])
def test_four_counted_barcodes(tmp_path, merge):
    rng = np.random.default_rng(52)
    s = readgen.make_set(rng, 3, 8, 3)
    counted = [readgen.make_set(rng, n, 8, 2) for n in (12, 9, 15)] + [readgen.make_set(rng, 10, 7, 2)]
    c = {"scheme": DEL4_SCHEME, "samples": {x: "S%d" % i for i, x in enumerate(s)}, "counted": counted, "kwargs": {},
         "reads": readgen.gen_reads(rng, DEL4_SCHEME, 3000, 110, s, counted, p_sub=0.01, p_n=0.002)}
    w = run_and_compare(tmp_path, c, unique_ids(c), merge)
    doubles = [f for f in w.files if ".Double." in f and ".all." not in f]
    assert doubles and all(len(w.files[f][1]) > 0 for f in doubles)


@pytest.mark.parametrize("merge", [False, True])
def test_random_barcode(tmp_path, merge):
    c = cases.build_case("del_random", seed=53, n=3000)
    run_and_compare(tmp_path, c, unique_ids(c), merge)


@pytest.mark.parametrize("merge", [False, True])
def test_sample_without_reads(tmp_path, merge):
    c = cases.build_case("del_mismatch_quality", seed=54, n=2000)
    c["samples"] = dict(c["samples"], TTTTTTTT="Z_no_reads")  # a sample no read carries
    w = run_and_compare(tmp_path, c, unique_ids(c), merge)
    for kind in ("Single", "Double"):
        fn = "enr_Z_no_reads_counts.%s.csv" % kind
        assert w.files[fn][1] == []
        assert open(os.path.join(str(tmp_path), "out", fn)).read() == "Barcode_1,Barcode_2,Barcode_3,Count\n"


def test_several_ranks(tmp_path):
    c = cases.build_case("del_mismatch_quality", seed=55, n=3001)
    run_and_compare(tmp_path, c, unique_ids(c), True, ["--gpus", "2", "--devices", "0,0", "--comm", "host"])


@pytest.mark.parametrize("name", ["raw_counted", "raw_sample"])
def test_raw_key_plans_keep_the_string_path(tmp_path, name):
    """plans whose keys are raw captures have no index form: their maps are still built from the rows' strings"""
    c = cases.build_case(name, seed=56, n=2000)
    tmp = str(tmp_path)
    args = write_plain_inputs(tmp, c)
    out = os.path.join(tmp, "out")
    os.makedirs(out)
    res = subprocess.run([CLI] + args + ["-o", out, "-p", "raw", "-e"], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, BC_ENRICH_VERBOSE="1"))
    assert res.returncode == 0, res.stderr + res.stdout
    assert "[barcode-count] enrichment: per-row string adds" in res.stderr, res.stderr[-500:]
    o, w = expected(c, "raw", False, True)
    assert sorted(f for f in os.listdir(out) if f.endswith(".csv")) == sorted(w.files)
    for fn, (header, rows) in w.files.items():
        assert read_csv(os.path.join(out, fn)) == (header, rows), fn
