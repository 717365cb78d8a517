"""`barcode-count` on raw-key plans with BC_DEVICE_RAW_WRITERS=1: the full-counts files are sorted and rendered on the
device (bc_engine_render_raw_counts / bc_engine_render_raw_merged) instead of going through per-row host strings.  Every
file against the reference's writers (tests/pyref_output.py) over the oracle's counts and against the host path (the
switch unset), whose lines come in no fixed order; two device runs byte for byte."""
import os

import pytest

import cases
import readgen
import raw_render_cases as rrc
import raw_render_lib as rrl
from test_gpu_cli import read_csv, write_inputs
from test_gpu_cli_render import CLOCK, HOST, compare_with_reference, full_counts_files, run_cli

pytestmark = pytest.mark.gpu

RAW_DEVICE = "[barcode-count] raw writers: device text (bc_engine_render_raw_counts)"
RAW_HOST = "[barcode-count] raw writers: per-row strings"
ON = {"BC_DEVICE_RAW_WRITERS": "1"}


def sample_file_raw_counted(n=4000, seed=71):
    """a sample file of 4, DEL_SCHEME, no counted file; captures from small pools, so that tuples repeat across samples"""
    import numpy as np
    rng = np.random.default_rng(seed)
    c = {"scheme": cases.DEL_SCHEME, "samples": {s: "Sample_%d" % i for i, s in enumerate(rrc.DEL_SAMPLES)}, "counted": None,
         "kwargs": {}}
    pool = [readgen.make_set(rng, 6, 8, 2) for _ in range(3)]
    c["reads"] = readgen.gen_reads(rng, cases.DEL_SCHEME, n, 100, rrc.DEL_SAMPLES, pool, p_sub=0.01, p_n=0.004)
    return c


def device_vs_host(tmp_path, c, merge, extra=()):
    tmp = str(tmp_path)
    args = write_inputs(tmp, c)
    out_d, res_d = run_cli(tmp, args, "dev", merge, False, extra, env=ON)
    assert RAW_DEVICE in res_d.stderr and HOST in res_d.stderr, res_d.stderr[-600:]  # (the first line is the dense path's)
    compare_with_reference(out_d, c, merge, False)
    out_h, res_h = run_cli(tmp, args, "host", merge, False, extra)
    assert RAW_HOST in res_h.stderr and HOST in res_h.stderr, res_h.stderr[-600:]
    # the same file set, headers and sorted lines; the same stdout and stats file up to the clock lines
    assert sorted(os.listdir(out_d)) == sorted(os.listdir(out_h))
    for f in os.listdir(out_d):
        if f.endswith(".csv"):
            assert read_csv(os.path.join(out_d, f)) == read_csv(os.path.join(out_h, f)), f
    mask = lambda text, out: CLOCK.sub("", text.replace(out, "<out>"))
    assert mask(res_d.stdout, out_d) == mask(res_h.stdout, out_h)
    stats = [mask(open(os.path.join(o, "r_barcode_stats.txt")).read(), o) for o in (out_d, out_h)]
    assert stats[0] == stats[1]
    # a second device run: byte for byte, the lines ascending by the digit tuple of their own text
    out_2, res_2 = run_cli(tmp, args, "dev2", merge, False, extra, env=ON)
    assert RAW_DEVICE in res_2.stderr
    files = full_counts_files(out_d)
    assert files
    G = sum(1 for k, _ in readgen.scheme_layout(c["scheme"]) if k == "B")
    for f in files:
        data = open(os.path.join(out_d, f), "rb").read()
        assert data == open(os.path.join(out_2, f), "rb").read(), f
        keys = [tuple(rrl.code_of(x) for x in line.split(",")[:G]) for line in data.decode().split("\n")[1:-1]]
        assert keys == sorted(keys) and len(set(keys)) == len(keys), f
    return out_d


@pytest.mark.parametrize("merge", [False, True])
def test_raw_counted(tmp_path, merge):
    c = cases.build_case("raw_counted", seed=67, n=1500)
    out = device_vs_host(tmp_path, c, merge)  # (-m with one key: "Merged file cannot be created", both paths)
    assert full_counts_files(out) == ["r_barcode_counts.csv"]
    assert len(open(os.path.join(out, "r_barcode_counts.csv")).read().split("\n")) > 20


@pytest.mark.parametrize("merge", [False, True])
def test_sample_file_and_raw_counted(tmp_path, merge):
    c = sample_file_raw_counted()
    out = device_vs_host(tmp_path, c, merge)
    assert len(full_counts_files(out)) == 4 + (1 if merge else 0)
    if merge:
        lines = open(os.path.join(out, "r_counts.all.csv")).read().split("\n")[1:-1]
        assert len(lines) > 50 and any(",0" in x for x in lines) and any(",0" not in x for x in lines)


def test_several_ranks(tmp_path):
    c = sample_file_raw_counted(n=4001, seed=72)
    device_vs_host(tmp_path, c, True, ["--gpus", "2", "--devices", "0,0", "--comm", "host"])


def test_enrichment_keeps_the_rows(tmp_path):
    """-e on a raw-key plan needs the rows' strings: the run stays on the host path, and writes what the reference writes"""
    c = sample_file_raw_counted(n=2000, seed=73)
    tmp = str(tmp_path)
    args = write_inputs(tmp, c)
    out, res = run_cli(tmp, args, "e", True, True, env=ON)
    assert RAW_HOST in res.stderr and RAW_DEVICE not in res.stderr
    compare_with_reference(out, c, True, True)


def test_default_is_the_host_path(tmp_path):
    c = cases.build_case("raw_counted", seed=67, n=600)
    tmp = str(tmp_path)
    out, res = run_cli(tmp, write_inputs(tmp, c), "d", False, False)
    assert RAW_HOST in res.stderr
    out, res = run_cli(tmp, write_inputs(tmp, c), "z", False, False, env={"BC_DEVICE_RAW_WRITERS": "0"})
    assert RAW_HOST in res.stderr
