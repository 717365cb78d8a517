"""The raw-key renderer's lane code on the host (tests/render/raw_render_host.cpp, under AddressSanitizer) and a Python
formatter of the same files, for tests/test_raw_render_emulation.py and the GPU tests of the renderer.

A plan's counted groups are described as `groups`: a list whose entry is an int L (a raw capture of L bases) or a list of
IDs (bytes; a known set).  A row is (s, digits, count): the sample index, one digit per group (set index, or the capture's
base-5 code with the first base least significant), the count."""
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "render", "raw_render_host")
SRC = os.path.join(ROOT, "tests", "render", "raw_render_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "tests", "render", "stage_check.h")] + [
    os.path.join(CSRC, h) for h in ("bc_raw_render.h", "bc_render.h", "bc_intrin.h")]
BASES = "ACTGN"


def exe():
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", EXE, SRC])
    return EXE


def radix(group):
    return 5 ** group if isinstance(group, int) else len(group)


def code_of(bases):
    """base-5 code of a capture: first base least significant"""
    return sum(BASES.index(c) * 5 ** k for k, c in enumerate(bases))


def field(group, digit):
    if isinstance(group, int):
        out = []
        for _ in range(group):
            out.append(BASES[digit % 5])
            digit //= 5
        return "".join(out).encode()
    return group[digit]


def tuple_number(groups, digits):
    t = 0
    for g, d in zip(groups, digits):
        assert 0 <= d < radix(g)
        t = t * radix(g) + d
    return t


def render_py(groups, rows, cols, merged):
    """-> (text, lines): the file of sample cols[0] (merged False) or the merged file of the columns `cols`"""
    by_tuple = {}
    for s, digits, count in rows:
        by_tuple.setdefault(tuple(digits), {})[s] = count
    out, lines = [], 0
    for digits in sorted(by_tuple):  # tuples of per-group digits, compared group by group
        per = by_tuple[digits]
        if merged:
            counts = [per.get(c, 0) for c in cols]
            if not any(counts):
                continue
        else:
            if cols[0] not in per:
                continue
            counts = [per[cols[0]]]
        out.append(b",".join([field(g, d) for g, d in zip(groups, digits)] + [b"%d" % c for c in counts]) + b"\n")
        lines += 1
    return b"".join(out), lines


def run(groups, rows, cols, merged, S, tmp_path, tag="case", win=4096, pad=0):
    """rows -> sorted (T * S + s, count) pairs -> (text, lines) from the harness"""
    pairs = sorted((tuple_number(groups, d) * S + s, c) for s, d, c in rows)
    assert all(k < 2 ** 64 for k, _ in pairs) and len({k for k, _ in pairs}) == len(pairs)
    fin, fout = os.path.join(str(tmp_path), tag + ".in"), os.path.join(str(tmp_path), tag + ".out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<6IQ", len(groups), len(cols), S, 1 if merged else 0, win, pad, len(pairs)))
        for g in groups:
            if isinstance(g, int):
                f.write(struct.pack("<2I", g, 0))
            else:
                f.write(struct.pack("<2I", 0, len(g)))
                for i in g:
                    f.write(struct.pack("<I", len(i)) + i)
        f.write(struct.pack("<%dI" % len(cols), *cols))
        f.write(struct.pack("<%dQ" % len(pairs), *[k for k, _ in pairs]))
        f.write(struct.pack("<%dI" % len(pairs), *[c for _, c in pairs]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe(), fin, fout], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and not p.stderr, "%s: exit %d\n%s" % (tag, p.returncode, p.stderr.decode(errors="replace")[-4000:])
    raw = open(fout, "rb").read()
    lines, nbytes = struct.unpack_from("<2Q", raw, 0)
    assert len(raw) == 16 + nbytes
    return raw[16:], lines
