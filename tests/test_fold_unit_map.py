"""How bc_fold_apply's workgroups share out the fold's units of work (csrc/bc_fold.h: fold_apply_unit), a unit being one
quarter of one item's bucket.  tests/fold/unit_map_host.cpp walks every grid from 1 to 600 workgroups over 0 to 1400
items as the kernel does and asserts that every (item, quarter) comes up exactly once and nothing else does, and that a
grid which is a multiple of 32 puts the four quarters of an item on blocks congruent mod 8 and in one step.  The function
runs on the host under AddressSanitizer and UndefinedBehaviorSanitizer, a child process with nothing preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "fold", "unit_map_host.cpp")
EXE = os.path.join(ROOT, "tests", "fold", "unit_map_host")
DEPS = [SRC, os.path.join(CSRC, "bc_fold.h"), os.path.join(CSRC, "bc_intrin.h")]


def test_every_unit_exactly_once_and_siblings_together():
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I" + CSRC, "-o", EXE, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([EXE], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and not p.stderr, "exit %d\n%s\n%s" % (p.returncode, out[-4000:], p.stderr.decode(errors="replace")[-4000:])
    assert out.strip().split("\n")[-1] == "ok 600 %d" % (600 * 17)
