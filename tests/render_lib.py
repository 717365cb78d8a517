"""Builds and runs tests/render/render_host: the text renderer's lane code (csrc/bc_render.h) on the host, compiled with
AddressSanitizer and UndefinedBehaviorSanitizer, as a child process; and the ten-line Python rendering every render test
compares with.  TEST-ONLY."""
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "render", "render_host")
SRC = os.path.join(ROOT, "tests", "render", "render_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "tests", "render", "stage_check.h"), os.path.join(CSRC, "bc_render.h"),
        os.path.join(CSRC, "bc_intrin.h")]


def exe():
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", EXE, SRC])
    return EXE


def render_py(ids, counts, cols):
    """ids: per counted barcode the list of IDs (bytes); counts[s][t]: the count of sample s, tuple t (t = the dense
    index, last barcode fastest); cols: sample indices -> (text, lines).  The definition the device code is held to."""
    sizes = [len(g) for g in ids]
    T = 1
    for n in sizes:
        T *= n
    out, lines = [], 0
    for t in range(T):
        cs = [int(counts[s][t]) for s in cols]
        if not any(cs):
            continue
        digits, r = [], t
        for n in reversed(sizes):
            digits.append(r % n)
            r //= n
        digits.reverse()
        out.append(b",".join([ids[g][d] for g, d in enumerate(digits)] + [str(c).encode() for c in cs]) + b"\n")
        lines += 1
    return b"".join(out), lines


def run(ids, table, n_samples, cols, tmp_path, tag="case", win=4096, pad=0, bits=None):
    """table: flat counts, sample-major (n_samples * T values) -> (text, lines) from the harness"""
    fin, fout = os.path.join(str(tmp_path), tag + ".in"), os.path.join(str(tmp_path), tag + ".out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<6I", len(ids), len(cols), n_samples, win, pad, 1 if bits is not None else 0))
        f.write(struct.pack("<%dI" % len(ids), *[len(g) for g in ids]))
        f.write(struct.pack("<%dI" % len(cols), *cols))
        for g in ids:
            for i in g:
                f.write(struct.pack("<I", len(i)) + i)
        f.write(struct.pack("<%dI" % len(table), *table))
        if bits is not None:
            f.write(struct.pack("<%dI" % len(bits), *bits))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe(), fin, fout], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and not p.stderr, "%s: exit %d\n%s" % (tag, p.returncode, p.stderr.decode(errors="replace")[-4000:])
    raw = open(fout, "rb").read()
    lines, nbytes = struct.unpack_from("<2Q", raw, 0)
    assert len(raw) == 16 + nbytes
    return raw[16:], lines
