"""`barcode-count -e`: the Single / Double files written from the device (bc_engine_render_enriched / _merged) against
the reference's writers (tests/pyref_output.py over the oracle's counts) and against the host path
(BC_DEVICE_ENRICH_WRITERS=0): the same files, the same sets of lines, the same stdout and stats file; on the device path
the lines come in ascending key order, byte for byte the same on every run."""
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import parity
import pyref_output
import readgen
from test_gpu_cli import CLI, canonical, read_csv, write_inputs

pytestmark = pytest.mark.gpu

W_DEVICE = "[barcode-count] writers: device text (bc_engine_render_counts)"
E_DEVICE = "[barcode-count] enrichment writers: device text (bc_engine_render_enriched)"
E_HOST = "[barcode-count] enrichment writers: per-row strings"
SUMS = "[barcode-count] enrichment: device marginal sums"
NO_MAPS = "[barcode-count] enrichment maps: 0 keys on the host"
CLOCK = re.compile(r"^(Start|Finish|Total time|Compute time).*$", re.M)


def default_id(b, i, s):
    return "bb%d_%s" % (b + 1, s)


def inputs(tmp, c, id_of):
    """tests/test_gpu_cli.write_inputs with the counted IDs chosen by id_of(barcode, index, sequence)"""
    args = write_inputs(tmp, c)
    if c.get("counted"):
        open(os.path.join(tmp, "counted.csv"), "w").write("Barcode,Barcode_ID,Barcode_Number\n" + "".join(
            "%s,%s,%d\n" % (s, id_of(b, i, s), b + 1) for b, refs in enumerate(c["counted"]) for i, s in enumerate(refs)))
    return args


def expected(c, merge, id_of):
    o = parity.oracle_for(c)
    for s, q in c["reads"]:
        o.process(s, q)
    results = {k: {} for k in o.sample_keys()}
    for s, t, n in o.rows():
        results.setdefault(s, {})[t] = n
    counted_hash = [{s: id_of(b, i, s) for i, s in enumerate(refs)} for b, refs in enumerate(c["counted"])] if c.get("counted") else []
    return o, pyref_output.Writer(results, dict(c["samples"] or {}), counted_hash, o.barcode_num, "r", merge, True).write()


def run_cli(tmp, args, tag, merge, extra=(), env=None, text=True):
    out = os.path.join(tmp, tag)
    os.makedirs(out)
    cmd = [CLI] + args + ["-o", out, "-p", "r", "-e"] + (["-m"] if merge else []) + list(extra)
    res = subprocess.run(cmd, capture_output=True, text=text, timeout=600,
                         env=dict(os.environ, BC_WRITERS_VERBOSE="1", BC_ENRICH_VERBOSE="1", **(env or {})))
    assert res.returncode == 0, res.stderr[-2000:]
    return out, res


def compare_with_reference(out, c, merge, id_of):
    o, w = expected(c, merge, id_of)
    produced = sorted(f for f in os.listdir(out) if f.endswith(".csv"))
    assert produced == sorted(w.files), (produced, sorted(w.files))
    assert any(".Single." in f for f in produced)
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


def key_index_of(line, c, id_of):
    """the key index of a Single / Double line (IDs must be distinct inside a set and free of commas)"""
    sets = [[id_of(b, i, s) for i, s in enumerate(refs)] for b, refs in enumerate(c["counted"])]
    G = len(sets)
    cells = line.split(",")[:G]
    held = [g for g in range(G) if cells[g] != ""]
    if len(held) == 1:
        g = held[0]
        return sum(len(x) for x in sets[:g]) + sets[g].index(cells[g])
    g, h = held
    base = sum(len(sets[a]) * len(sets[b]) for a in range(G) for b in range(a + 1, G) if (a, b) < (g, h))
    return base + sets[g].index(cells[g]) * len(sets[h]) + sets[h].index(cells[h])


def device_vs_host(tmp_path, c, merge, extra=(), id_of=default_id, expect_device=True, ordered=True):
    tmp = str(tmp_path)
    args = inputs(tmp, c, id_of)
    out_d, res_d = run_cli(tmp, args, "dev", merge, extra)
    assert (E_DEVICE if expect_device else E_HOST) in res_d.stderr, res_d.stderr[-600:]
    if expect_device:
        assert W_DEVICE in res_d.stderr and SUMS in res_d.stderr, res_d.stderr[-600:]
    # the device path builds neither single_hash nor double_hash (no fill_enrichment, no per-row adds); the host path does
    assert (NO_MAPS in res_d.stderr) == expect_device, res_d.stderr[-600:]
    compare_with_reference(out_d, c, merge, id_of)
    out_h, res_h = run_cli(tmp, args, "host", merge, extra, env={"BC_DEVICE_ENRICH_WRITERS": "0"})
    assert E_HOST in res_h.stderr and "enrichment maps: " in res_h.stderr and NO_MAPS not in res_h.stderr, res_h.stderr[-600:]
    if expect_device:
        assert W_DEVICE in res_h.stderr  # (the counts files stay on the device)
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
    # a second device-path run: the Single / Double files byte for byte, their lines in ascending key order
    out_2, res_2 = run_cli(tmp, args, "dev2", merge, extra)
    assert E_DEVICE in res_2.stderr
    files = sorted(f for f in os.listdir(out_d) if ".Single." in f or ".Double." in f)
    assert files
    for f in files:
        data = open(os.path.join(out_d, f), "rb").read()
        assert data == open(os.path.join(out_2, f), "rb").read(), f
        if ordered:
            idx = [key_index_of(line, c, id_of) for line in data.decode().split("\n")[1:-1]]
            assert idx == sorted(idx) and len(set(idx)) == len(idx), f
    return out_d


@pytest.mark.parametrize("merge", [False, True])
def test_del(tmp_path, merge):
    c = cases.build_case("del_mismatch_quality", seed=71, n=3000)
    out = device_vs_host(tmp_path, c, merge)
    assert any(".Double." in f for f in os.listdir(out))


def test_four_counted_barcodes(tmp_path):
    rng = np.random.default_rng(72)
    scheme = "[6]AGCTAGATC{5}TGGA{5}TGAT{5}TGCA{5}CTAGCA"
    s = readgen.make_set(rng, 3, 6, 2)
    c = dict(name="four", kwargs={}, scheme=scheme, samples={x: "S%d" % i for i, x in enumerate(s)},
             counted=[readgen.make_set(rng, 6 + g, 5, 2) for g in range(4)])
    c["reads"] = readgen.gen_reads(rng, scheme, 3000, 60, s, c["counted"], p_sub=0.01, p_n=0.002)
    out = device_vs_host(tmp_path, c, True)
    double = open(os.path.join(out, "r_counts.all.Double.csv")).read().split("\n")
    assert double[0].startswith("Barcode_1,Barcode_2,Barcode_3,Barcode_4,") and len(double) > 50
    assert all(sum(1 for x in line.split(",")[:4] if x) == 2 for line in double[1:-1])


def test_random_barcode(tmp_path):
    c = cases.build_case("del_random", seed=73, n=3000)
    device_vs_host(tmp_path, c, True)


def test_ids_shared_inside_a_group(tmp_path):
    c = cases.build_case("del_mismatch_quality", seed=74, n=3000)
    shared = lambda b, i, s: "bb%d_%d" % (b + 1, i % 7 if b != 1 else i)  # sets 0 and 2: seven IDs for sixty sequences
    out = device_vs_host(tmp_path, c, True, id_of=shared, ordered=False)
    single = open(os.path.join(out, "r_counts.all.Single.csv")).read().split("\n")[1:-1]
    assert len(single) <= 7 + 60 + 7 and len(set(x.rsplit(",", 4)[0] for x in single)) == len(single)


def test_sample_without_reads(tmp_path):
    c = cases.build_case("del_mismatch_quality", seed=75, n=2000)
    c["samples"] = dict(c["samples"], TTTTTTTT="Z_no_reads")
    out = device_vs_host(tmp_path, c, True)
    for kind in ("Single", "Double"):
        assert open(os.path.join(out, "r_Z_no_reads_counts.%s.csv" % kind)).read() == "Barcode_1,Barcode_2,Barcode_3,Count\n"


def test_several_ranks(tmp_path):
    c = cases.build_case("del_mismatch_quality", seed=76, n=3001)
    device_vs_host(tmp_path, c, True, ["--gpus", "2", "--devices", "0,0", "--comm", "host"])


def test_an_empty_id_keeps_the_host_path(tmp_path):
    """",," is then the text of keys in different groups: the reference adds them up, the device's key space does not"""
    c = cases.build_case("del_mismatch_quality", seed=77, n=2500)
    one_empty = lambda b, i, s: "" if (b, i) == (1, 3) else default_id(b, i, s)
    device_vs_host(tmp_path, c, True, id_of=one_empty, expect_device=False)


def test_raw_keys_keep_the_host_path(tmp_path):
    c = cases.build_case("raw_counted", seed=78, n=1500)
    device_vs_host(tmp_path, c, False, expect_device=False)


def test_progress_lines_of_a_file_above_50_000_lines(tmp_path):
    """add_counts_string prints `Barcodes counted: N\\r` every 50,000 rows of a Single / Double file too; the device path
    prints the same bytes from the line count.  2 x 3 x 140^2 pairs per sample, 400,000 reads: every sample's Double file
    passes 50,000 lines."""
    import workloads
    w = workloads.make("config3", n_sets=(2, 140, 140, 140))
    n, R = 400_000, w.read_len
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
    out_d, res_d = run_cli(tmp, args, "dev", True, text=False)
    out_h, res_h = run_cli(tmp, args, "host", True, env={"BC_DEVICE_ENRICH_WRITERS": "0"}, text=False)
    assert E_DEVICE.encode() in res_d.stderr and E_HOST.encode() in res_h.stderr
    # stdout as bytes: the progress lines end in a carriage return, not a newline
    clock = re.compile(CLOCK.pattern.encode(), re.M)
    assert clock.sub(b"", res_d.stdout) == clock.sub(b"", res_h.stdout)
    for s in range(2):
        assert b"r_sample_%d_counts.Double.csv\nBarcodes counted: 50,000\rBarcodes counted: 5" % s in res_d.stdout, res_d.stdout[-800:]
    for f in os.listdir(out_d):
        if f.endswith(".csv"):
            assert read_csv(os.path.join(out_d, f)) == read_csv(os.path.join(out_h, f)), f
            if ".Double." in f:
                assert len(read_csv(os.path.join(out_d, f))[1]) > 50_000, f
