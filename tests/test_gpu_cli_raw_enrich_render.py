"""`barcode-count -e` on raw-key plans with BC_DEVICE_RAW_WRITERS=1 and BC_DEVICE_RAW_ENRICH_WRITERS=1: the Single and
Double files, like the full-counts files, are summed, sorted and rendered on the device
(bc_engine_render_raw_enriched / _merged) and no row becomes a host string.  Every file against the reference's writers
(tests/pyref_output.py) over the oracle's counts and against the host path (the switches unset) of the same binary,
whose lines come in no fixed order; two device runs byte for byte."""
import os

import pytest

import cases
import test_gpu_cli_enrich_render as er
from test_gpu_cli import read_csv, write_inputs
from test_gpu_cli_raw_render import RAW_DEVICE, RAW_HOST, sample_file_raw_counted
from test_gpu_cli_render import CLOCK, compare_with_reference, run_cli

pytestmark = pytest.mark.gpu

ENRICH_DEVICE = "[barcode-count] enrichment writers: device text (bc_engine_render_raw_enriched)"
ENRICH_HOST = "[barcode-count] enrichment writers: per-row strings"
NO_KEYS = "[barcode-count] enrichment maps: 0 keys on the host"
ON = {"BC_DEVICE_RAW_WRITERS": "1", "BC_DEVICE_RAW_ENRICH_WRITERS": "1"}


def device_vs_host(tmp_path, c, merge, extra=()):
    tmp = str(tmp_path)
    args = write_inputs(tmp, c)
    out_d, res_d = run_cli(tmp, args, "dev", merge, True, extra, env=ON)
    assert RAW_DEVICE in res_d.stderr and ENRICH_DEVICE in res_d.stderr and NO_KEYS in res_d.stderr, res_d.stderr[-800:]
    compare_with_reference(out_d, c, merge, True)
    out_h, res_h = run_cli(tmp, args, "host", merge, True, extra)
    assert RAW_HOST in res_h.stderr and ENRICH_HOST in res_h.stderr and NO_KEYS not in res_h.stderr, res_h.stderr[-800:]
    # the same file set, headers and sorted lines; the same stdout and stats file up to the clock lines
    assert sorted(os.listdir(out_d)) == sorted(os.listdir(out_h))
    enriched = [f for f in os.listdir(out_d) if ".Single." in f or ".Double." in f]
    assert len(enriched) == 2 * (4 + (1 if merge else 0))
    for f in os.listdir(out_d):
        if f.endswith(".csv"):
            assert read_csv(os.path.join(out_d, f)) == read_csv(os.path.join(out_h, f)), f
    mask = lambda text, out: CLOCK.sub("", text.replace(out, "<out>"))
    assert mask(res_d.stdout, out_d) == mask(res_h.stdout, out_h)
    stats = [mask(open(os.path.join(o, "r_barcode_stats.txt")).read(), o) for o in (out_d, out_h)]
    assert stats[0] == stats[1]
    # a second device run: byte for byte
    out_2, res_2 = run_cli(tmp, args, "dev2", merge, True, extra, env=ON)
    assert ENRICH_DEVICE in res_2.stderr
    for f in os.listdir(out_d):
        if f.endswith(".csv"):
            data = open(os.path.join(out_d, f), "rb").read()
            assert data == open(os.path.join(out_2, f), "rb").read(), f
            assert len(data.split(b"\n")) > 5, f
    return out_d


@pytest.mark.parametrize("merge", [False, True])
def test_sample_file_and_raw_counted(tmp_path, merge):
    device_vs_host(tmp_path, sample_file_raw_counted(), merge)


def test_several_ranks(tmp_path):
    device_vs_host(tmp_path, sample_file_raw_counted(n=4001, seed=72), True, ["--gpus", "2", "--devices", "0,0", "--comm", "host"])


def test_the_enrichment_switch_alone_keeps_the_rows(tmp_path):
    """BC_DEVICE_RAW_ENRICH_WRITERS=1 means something only on top of BC_DEVICE_RAW_WRITERS=1"""
    c = sample_file_raw_counted(n=2000, seed=73)
    tmp = str(tmp_path)
    out, res = run_cli(tmp, write_inputs(tmp, c), "e", True, True, env={"BC_DEVICE_RAW_ENRICH_WRITERS": "1"})
    assert RAW_HOST in res.stderr and ENRICH_HOST in res.stderr and ENRICH_DEVICE not in res.stderr
    compare_with_reference(out, c, True, True)
    out, res = run_cli(tmp, write_inputs(tmp, c), "z", True, True, env=dict(ON, BC_DEVICE_RAW_ENRICH_WRITERS="0"))
    assert RAW_HOST in res.stderr and ENRICH_HOST in res.stderr and ENRICH_DEVICE not in res.stderr
    compare_with_reference(out, c, True, True)


@pytest.mark.parametrize("name", ["raw_sample", "del_mismatch_quality"])
def test_an_empty_id_keeps_the_rows(tmp_path, name):
    """Both switches on and a counted file in which one ID is empty.  IDs exist only where the counted file names every
    barcode, and such a plan is never on the raw-key device path: either its sample barcode is kept raw ("raw_sample",
    a raw-key plan whose samples are captures) or it is a dense plan ("del_mismatch_quality", whose own enrichment
    writers refuse an empty ID).  Either way the Single / Double files come from per-row strings and are the
    reference's."""
    c = cases.build_case(name, seed=79, n=2000)
    one_empty = lambda b, i, s: "" if (b, i) == (1, 3) else er.default_id(b, i, s)
    tmp = str(tmp_path)
    merge = bool(c.get("samples"))
    out, res = er.run_cli(tmp, er.inputs(tmp, c, one_empty), "e", merge, env=ON)
    assert ENRICH_HOST in res.stderr and ENRICH_DEVICE not in res.stderr and NO_KEYS not in res.stderr, res.stderr[-800:]
    assert (RAW_HOST in res.stderr) == (name == "raw_sample") and RAW_DEVICE not in res.stderr
    er.compare_with_reference(out, c, merge, one_empty)
    single = [f for f in os.listdir(out) if ".Single." in f]
    assert single and any(",," in line for f in single for line in open(os.path.join(out, f)).read().split("\n")[1:])
