"""Builds and runs tests/ingest/ingest_host: the FASTQ ingest's host-only logic (csrc/bc_fastq_host.hpp), compiled with
AddressSanitizer and UndefinedBehaviorSanitizer, as a child process.  TEST-ONLY."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "ingest", "ingest_host")
SRC = os.path.join(ROOT, "tests", "ingest", "ingest_host.cpp")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("bc_fastq_host.hpp", "bc_bgzf.hpp")]


def exe():
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-fno-omit-frame-pointer", "-o", EXE, SRC])
    return EXE


def hexed(data):
    return data.hex() if data else "-"


def ask(tmp_path, queries):
    """the answer lines of ingest_host to the query lines, one each; the run must be clean under the sanitizers"""
    qin, qout = os.path.join(str(tmp_path), "queries.in"), os.path.join(str(tmp_path), "queries.out")
    with open(qin, "w") as f:
        f.write("".join(q + "\n" for q in queries))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe(), qin, qout], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and not p.stderr, "exit %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-4000:])
    answers = open(qout).read().split("\n")[:-1]
    assert len(answers) == len(queries)
    return answers
