"""The raw-key enrichment renderer's lane code on the host (tests/render/raw_enrich_render_host.cpp, under
AddressSanitizer + UBSan) and a Python formatter of the same files, for tests/test_raw_enrich_render_emulation.py and the
GPU tests of the renderer.

Groups and rows are described as tests/raw_render_lib.py describes them: a group is an int L (a raw capture of L bases)
or a list of IDs (bytes; a known set); a row is (s, digits, count).  The formatter builds the Single / Double maps from
the rows the way add_single / add_double do (info.rs:840-904): one dict per kind, keyed by (group or pair, the digits
kept), to which every row adds its count under its sample -- entries of a known set that carry the same ID being one
key, because the reference's keys are text."""
import os
import struct
import subprocess

import raw_render_lib as rrl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "render", "raw_enrich_render_host")
SRC = os.path.join(ROOT, "tests", "render", "raw_enrich_render_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "tests", "render", "stage_check.h")] + [
    os.path.join(CSRC, h) for h in ("bc_raw_enrich_render.h", "bc_enrich_render.h", "bc_raw_render.h", "bc_render.h", "bc_intrin.h")]
SINGLE, DOUBLE = 1, 2


def exe():
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", EXE, SRC])
    return EXE


def canon(group, digit):
    """the digit a key is made of: of a known set the smallest index that carries the same ID"""
    return digit if isinstance(group, int) else group.index(group[digit])


def maps_of(groups, rows, kind):
    """{(fields, digits): {s: sum}} with fields = (g,) or (g, h), as add_single / add_double fill their maps"""
    G = len(groups)
    fields = [(g,) for g in range(G)] if kind == SINGLE else [(g, h) for g in range(G) for h in range(g + 1, G)]
    if kind == DOUBLE and G < 3:
        fields = []  # (the reference makes no Double file below three counted barcodes)
    maps = {}
    for s, digits, count in rows:
        for fs in fields:
            per = maps.setdefault((fs, tuple(canon(groups[f], digits[f]) for f in fs)), {})
            per[s] = per.get(s, 0) + count
    return maps


def render_py(groups, rows, cols, merged, kind):
    """-> (text, lines): the Single / Double file of sample cols[0] (merged False) or the merged one of the columns `cols`;
    lines ascend by (group or pair, digits)"""
    maps = maps_of(groups, rows, kind)
    out = []
    for fs, ds in sorted(maps):
        per = maps[(fs, ds)]
        if merged:
            counts = [per.get(c, 0) for c in cols]
            if not any(counts):
                continue
        else:
            if cols[0] not in per:
                continue
            counts = [per[cols[0]]]
        text = [b""] * len(groups)
        for f, d in zip(fs, ds):
            text[f] = rrl.field(groups[f], d)
        out.append(b",".join(text + [b"%d" % c for c in counts]) + b"\n")
    return b"".join(out), len(out)


def run(groups, rows, cols, merged, kind, S, tmp_path, tag="case", win=4096, pad=0):
    """rows -> sorted (T * S + s, count) pairs -> (text, lines) from the harness"""
    pairs = sorted((rrl.tuple_number(groups, d) * S + s, c) for s, d, c in rows)
    assert all(k < 2 ** 64 for k, _ in pairs) and len({k for k, _ in pairs}) == len(pairs)
    fin, fout = os.path.join(str(tmp_path), tag + ".in"), os.path.join(str(tmp_path), tag + ".out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<8IQ", len(groups), len(cols), S, 1 if merged else 0, win, pad, kind, 0, len(pairs)))
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
