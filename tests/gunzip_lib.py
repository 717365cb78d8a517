"""Builds and runs tests/gunzip/gunzip_host: the span inflater's lane code (csrc/bc_gunzip.h) on the host, compiled with
AddressSanitizer and UndefinedBehaviorSanitizer, as a child process.  TEST-ONLY."""
import itertools
import os
import subprocess

import gunzip_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "gunzip", "gunzip_host")
SRC = os.path.join(ROOT, "tests", "gunzip", "gunzip_host.cpp")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("bc_gunzip.h", "bc_inflate.h", "bc_intrin.h")]
_serial = itertools.count()


def exe():
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", EXE, SRC])
    return EXE


def runner(tmp_path):
    """-> run(src, start_bit, hist, capacity, part_bytes) of gunzip_cases, through the host build"""
    def run(src, start_bit, hist, capacity, part_bytes):
        tag = os.path.join(str(tmp_path), "span%d" % next(_serial))
        with open(tag + ".in", "wb") as f:
            f.write(gunzip_cases.pack_input(src, start_bit, hist, capacity, part_bytes))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe(), tag + ".in", tag + ".out"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0 and not p.stderr, "exit %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-4000:])
        raw = open(tag + ".out", "rb").read()
        os.unlink(tag + ".in")
        os.unlink(tag + ".out")
        r, image = gunzip_cases.unpack_output(raw)
        assert len(image) == capacity
        return r, image
    return run
