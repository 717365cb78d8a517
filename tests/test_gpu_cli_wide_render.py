"""`barcode-count` on wide-key plans (captures above 27 bases without a conversion file) with BC_DEVICE_RAW_WRITERS=1: the
full-counts files are sorted and rendered on the device (bc_engine_render_wide_counts / bc_engine_render_wide_merged)
instead of going through per-row host strings.  Every file against the host path (the switch unset), whose lines come in
no fixed order: the same header and the same set of lines, the same stdout and stats file; the device's lines ascend by
the digit tuple of their own text."""
import os

import numpy as np
import pytest

import raw_render_lib as rrl
import readgen
import test_gpu_wide_keys as wk
from test_gpu_cli import read_csv, write_inputs
from test_gpu_cli_render import CLOCK, HOST, full_counts_files, run_cli

pytestmark = pytest.mark.gpu

WIDE_DEVICE = "[barcode-count] raw writers: device text (bc_engine_render_wide_counts)"
RAW_HOST = "[barcode-count] raw writers: per-row strings"
ON = {"BC_DEVICE_RAW_WRITERS": "1"}


def case(name, n, seed):
    """a test_gpu_wide_keys workload as the command line's inputs: a FASTQ, the scheme, the sample file when it has one"""
    c = wk.CASES[name]
    rng = np.random.default_rng(seed + 1000)
    pools = [wk._pool(rng, k, ln) for k, ln in c["pools"]]
    reads = wk._reads(c["parts"], n, seed, pools)
    samples = {s: "sample_%d" % i for i, s in enumerate(pools[c["samples_from"]])} if "samples_from" in c else None
    return {"scheme": c["scheme"], "samples": samples, "counted": None, "kwargs": {}, "reads": [(r, "I" * len(r)) for r in reads]}


def device_vs_host(tmp_path, c, merge, extra=(), host_extra=None):
    tmp = str(tmp_path)
    args = write_inputs(tmp, c)
    out_d, res_d = run_cli(tmp, args, "dev", merge, False, extra, env=ON)
    assert WIDE_DEVICE in res_d.stderr and HOST in res_d.stderr, res_d.stderr[-600:]  # (the first line is the dense path's)
    out_h, res_h = run_cli(tmp, args, "host", merge, False, extra if host_extra is None else host_extra)
    assert RAW_HOST in res_h.stderr and HOST in res_h.stderr, res_h.stderr[-600:]
    # the same file set, headers and sets of lines; for the same command line the same stdout and stats file up to the
    # clock lines
    assert sorted(os.listdir(out_d)) == sorted(os.listdir(out_h))
    for f in os.listdir(out_d):
        if f.endswith(".csv"):
            assert read_csv(os.path.join(out_d, f)) == read_csv(os.path.join(out_h, f)), f
    if host_extra is None:
        mask = lambda text, out: CLOCK.sub("", text.replace(out, "<out>"))
        assert mask(res_d.stdout, out_d) == mask(res_h.stdout, out_h)
        stats = [mask(open(os.path.join(o, "r_barcode_stats.txt")).read(), o) for o in (out_d, out_h)]
        assert stats[0] == stats[1]
    # the device's lines ascend by the digit tuple of their own text
    files = full_counts_files(out_d)
    assert files
    G = sum(1 for k, _ in readgen.scheme_layout(c["scheme"]) if k == "B")
    for f in files:
        lines = open(os.path.join(out_d, f)).read().split("\n")[1:-1]
        keys = [tuple(rrl.code_of(x) for x in line.split(",")[:G]) for line in lines]
        assert keys == sorted(keys) and len(set(keys)) == len(keys), f
    return out_d


def test_barcode_seq_40(tmp_path):
    """no sample file, no counted file: one file, a line per lineage barcode"""
    out = device_vs_host(tmp_path, case("barcode_seq_40", 3000, 31), False)
    assert full_counts_files(out) == ["r_barcode_counts.csv"]
    assert len(open(os.path.join(out, "r_barcode_counts.csv")).read().split("\n")) > 500


def test_samples_and_35_bases_merged(tmp_path):
    out = device_vs_host(tmp_path, case("samples_plus_raw_35", 3000, 33), True)
    assert len(full_counts_files(out)) == 5 + 1
    lines = open(os.path.join(out, "r_counts.all.csv")).read().split("\n")[1:-1]
    assert len(lines) > 300 and any(",0" in x for x in lines) and any(",0" not in x for x in lines)


def test_two_ranks_against_one_process(tmp_path):
    """--gpus 2 on the device path against the one-process host path: rank 0 renders what bc_engine_finish_all merged"""
    device_vs_host(tmp_path, case("barcode_seq_40", 3001, 35), False, ["--gpus", "2", "--devices", "0,0", "--comm", "host"], host_extra=[])


def test_enrichment_keeps_the_rows(tmp_path):
    """-e needs the rows' strings: a wide-key run with two counted barcodes stays on the host path"""
    parts = [("const", "CCTAGG"), ("cap", 24, 0), ("const", "AATT"), ("cap", 28, 1), ("const", "GGATCC")]
    rng = np.random.default_rng(37)
    pools = [wk._pool(rng, 6, 24), wk._pool(rng, 9, 28)]
    reads = wk._reads(parts, 1200, 37, pools)
    c = {"scheme": "CCTAGG{24}AATT{28}GGATCC", "samples": None, "counted": None, "kwargs": {},
         "reads": [(r, "I" * len(r)) for r in reads]}
    tmp = str(tmp_path)
    args = write_inputs(tmp, c)
    out_e, res = run_cli(tmp, args, "e", False, True, env=ON)
    assert RAW_HOST in res.stderr and WIDE_DEVICE not in res.stderr
    out_h, res_h = run_cli(tmp, args, "h", False, True)
    assert RAW_HOST in res_h.stderr
    assert sorted(os.listdir(out_e)) == sorted(os.listdir(out_h)) and len(os.listdir(out_e)) >= 3
    for f in os.listdir(out_e):
        if f.endswith(".csv"):
            assert read_csv(os.path.join(out_e, f)) == read_csv(os.path.join(out_h, f)), f
