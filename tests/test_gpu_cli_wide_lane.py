"""`barcode-count` on a wide-key plan (Barcode-seq with a 30-base lineage barcode, no conversion file) with BC_WIDE_LANE=0
and =1: the switch picks the kernel and nothing else -- the same counts files (their lines as sets: the order of rows
out of a hash map is not promised on the host path) and the same stdout up to the clock lines."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_gpu_wide_keys as twk
from test_gpu_cli import CLI, read_csv, write_inputs

pytestmark = pytest.mark.gpu
CLOCK = re.compile(r"^(Start|Finish|Total time|Compute time).*$", re.M)
SCHEME = "GTACCAGTC{30}TGCATGGAC"
PARTS = [("const", "GTACCAGTC"), ("cap", 30, 0), ("const", "TGCATGGAC")]


def test_switch_changes_no_output(tmp_path):
    rng = np.random.default_rng(51)
    reads = twk._reads(PARTS, 3000, 51, [twk._pool(rng, 400, 30)])
    c = dict(scheme=SCHEME, reads=[(r, "I" * len(r)) for r in reads])
    tmp = str(tmp_path)
    args = write_inputs(tmp, c)
    runs = {}
    for switch in ("0", "1"):
        out = os.path.join(tmp, "out" + switch)
        os.makedirs(out)
        res = subprocess.run([CLI] + args + ["-o", out, "-p", "r"], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, BC_WIDE_LANE=switch))
        assert res.returncode == 0, res.stderr + res.stdout
        files = sorted(f for f in os.listdir(out) if f.endswith(".csv"))
        runs[switch] = (files, [read_csv(os.path.join(out, f)) for f in files], CLOCK.sub("", res.stdout.replace(out, "<out>")))
    assert runs["0"] == runs["1"]
    files, tables, stdout = runs["1"]
    assert files and sum(len(rows) for _, rows in tables) > 300
    o = twk.oracle_lib.Oracle(SCHEME)
    for r in reads:
        o.process(r)
    assert sorted(line for _, rows in tables for line in rows) == sorted("%s,%d" % (t, n) for _, t, n in o.rows())
    assert "{:,}".format(o.counters["matched"]) in stdout or str(o.counters["matched"]) in stdout
