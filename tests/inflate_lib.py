"""Builds and runs tests/inflate/inflate_host: the device inflater's decoder (csrc/bc_inflate.h) on the host, compiled
with AddressSanitizer and UndefinedBehaviorSanitizer, as a child process.  TEST-ONLY."""
import os
import struct
import subprocess

import inflate_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "inflate", "inflate_host")
SRC = os.path.join(ROOT, "tests", "inflate", "inflate_host.cpp")
DEPS = [SRC, os.path.join(CSRC, "bc_inflate.h"), os.path.join(CSRC, "bc_intrin.h")]


def exe():
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", EXE, SRC])
    return EXE


def run(blocks, tmp_path, tag="case"):
    """-> (status words, output image) of the blocks of one case"""
    src, table, dst_bytes = inflate_cases.layout(blocks)
    fin, fout = os.path.join(str(tmp_path), tag + ".in"), os.path.join(str(tmp_path), tag + ".out")
    with open(fin, "wb") as f:
        f.write(inflate_cases.pack(src, table, dst_bytes))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe(), fin, fout], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and not p.stderr, "%s: exit %d\n%s" % (tag, p.returncode, p.stderr.decode(errors="replace")[-4000:])
    raw = open(fout, "rb").read()
    status = list(struct.unpack_from("<%dI" % len(table), raw, 0))
    return table, status, raw[4 * len(table):]
