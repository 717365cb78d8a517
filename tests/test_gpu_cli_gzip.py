"""`barcode-count` on an ordinary .fastq.gz with BC_GZ_DEVICE=all and with BC_GZ_DEVICE=1: the same stdout blocks and
the same files, byte for byte."""
import os
import re
import subprocess

import pytest

import gzip_ingest_files as files
from test_gpu_cli import CLI, write_inputs

pytestmark = pytest.mark.gpu


def run_cli(tmp, fq, args, mode):
    out = os.path.join(tmp, "out_" + mode)
    os.makedirs(out)
    env = dict(os.environ, BC_GZ_DEVICE=mode, BC_INGEST_VERBOSE="1", **files.ENV)
    res = subprocess.run([CLI, "-f", fq] + args + ["-o", out, "-p", "run", "-m", "-e"], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0, res.stderr + res.stdout
    # (the two time lines and the stats file's time block are the only text that may differ)
    stdout = re.sub(r"(Compute|Total) time: .*", r"\1 time: -", res.stdout)
    # the progress counter rewrites its line once per chunk ('\r', which text mode hands over as a line end), and the two
    # paths cut chunks differently: of a run of "Total sequences" lines the last one, the total itself, has to agree
    lines = stdout.split("\n")
    stdout = "\n".join(line for i, line in enumerate(lines)
                       if not (line.startswith("Total sequences:") and lines[i + 1].startswith("Total sequences:")))
    produced = {}
    for fn in sorted(os.listdir(out)):
        data = open(os.path.join(out, fn), "rb").read()
        if fn.endswith("_barcode_stats.txt"):
            data = re.sub(rb"(Start|Finish|Compute time|Total time): .*", rb"\1: -", data)
        produced[fn] = data
    return stdout, produced, res.stderr


def test_cli_gzip_device_equals_zlib(tmp_path):
    c = files.case()
    tmp = str(tmp_path)
    args = write_inputs(tmp, dict(c, reads=c["reads"][:10]), gz=True)[2:]  # (the scheme and CSV arguments; the reads follow)
    fq = files.write(tmp, "reads", files.variants()["no_final_newline"])
    out_dev, files_dev, err_dev = run_cli(tmp, fq, args, "all")
    out_zlib, files_zlib, err_zlib = run_cli(tmp, fq, args, "1")
    assert "path gzip-device" in err_dev and "path gzread" in err_zlib
    assert re.search(r"[1-9]\d* spans, [1-9]\d* segments, \d+ candidates rejected, \d+ retries", err_dev), err_dev
    assert out_dev == out_zlib
    assert "Total sequences:             {:,}".format(files.N_READS + 1) in out_dev
    assert sorted(files_dev) == sorted(files_zlib) and len(files_dev) >= 3
    for fn in files_dev:
        assert files_dev[fn] == files_zlib[fn], fn
