"""The wide-key renderer's lane code on the host (tests/render/wide_render_host.cpp, under AddressSanitizer + UBSan), for
tests/test_wide_render_emulation.py.  The Python formatter and the order are raw_render_lib's (render_py, code_of), whose
integers have any size.

A plan's counted groups are described as `groups`: a list whose entry is an int L (a raw capture of L bases) or a list of
IDs (bytes; a known set).  A row is (s, fields, count): the sample index, one field per group (the capture as a str of
ACTGN, or the set index), the count.  The payload is laid out as the plan layer lays it out (csrc/bc_plan.cpp): the
sample index first (32 bits, when the scheme has a sample group), then group after group 32 bits of index or the three
bit planes of a capture (ASCII bit 1, ASCII bit 2, 'N'), then `tail_bits` of zeros (a random barcode's cleared planes)."""
import os
import random
import struct
import subprocess

import raw_render_lib as rrl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "render", "wide_render_host")
SRC = os.path.join(ROOT, "tests", "render", "wide_render_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "tests", "render", "stage_check.h")] + [
    os.path.join(CSRC, h) for h in ("bc_wide_render.h", "bc_raw_render.h", "bc_render.h", "bc_intrin.h")]


def exe():
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", EXE, SRC])
    return EXE


def layout(groups, has_sample, tail_bits=0):
    """-> (key_bit of every group, payload words)"""
    bit = 32 if has_sample else 0
    key_bit = []
    for g in groups:
        key_bit.append(bit)
        bit += 3 * g if isinstance(g, int) else 32
    bit += tail_bits
    return key_bit, max(1, (bit + 63) // 64)


def payload(groups, key_bit, has_sample, s, fields):
    x = s if has_sample else 0
    for g, at, f in zip(groups, key_bit, fields):
        if isinstance(g, int):
            assert len(f) == g
            for k, c in enumerate(f):
                if c == "N":
                    x |= 1 << (at + 2 * g + k)
                else:
                    x |= ((ord(c) >> 1) & 1) << (at + k)
                    x |= ((ord(c) >> 2) & 1) << (at + g + k)
        else:
            x |= f << at
    return x


def digits(groups, fields):
    return tuple(rrl.code_of(f) if isinstance(g, int) else f for g, f in zip(groups, fields))


def order_bits(groups, S, has_sample):
    """bits of the order key: the sample's, then every group's"""
    return ((S - 1).bit_length() if has_sample else 0) + sum(3 * g if isinstance(g, int) else (len(g) - 1).bit_length() for g in groups)


def run(groups, rows, cols, merged, S, has_sample, tmp_path, tag="case", win=4096, pad=0, tail_bits=0, seed=1):
    """rows (in a shuffled order) -> (text, lines, order keys as Python integers in the rows' order) from the harness"""
    key_bit, words = layout(groups, has_sample, tail_bits)
    W = words + 1
    rng = random.Random(seed)
    rows = list(rows)
    rng.shuffle(rows)
    fin, fout, ford = (os.path.join(str(tmp_path), tag + e) for e in (".in", ".out", ".ord"))
    with open(fin, "wb") as f:
        f.write(struct.pack("<8IQ", len(groups), len(cols), S, 1 if merged else 0, win, pad, W, 1 if has_sample else 0, len(rows)))
        for g, at in zip(groups, key_bit):
            if isinstance(g, int):
                f.write(struct.pack("<3I", g, 0, at))
            else:
                f.write(struct.pack("<3I", 0, len(g), at))
                for i in g:
                    f.write(struct.pack("<I", len(i)) + i)
        f.write(struct.pack("<%dI" % len(cols), *cols))
        for s, fields, _ in rows:
            p = payload(groups, key_bit, has_sample, s, fields)
            assert p < 1 << (64 * words)
            f.write(struct.pack("<Q", rng.getrandbits(63)))  # word 0: a fingerprint nobody may look at
            f.write(struct.pack("<%dQ" % words, *[(p >> (64 * w)) & (2 ** 64 - 1) for w in range(words)]))
        f.write(struct.pack("<%dI" % len(rows), *[c for _, _, c in rows]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe(), fin, fout, ford], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and not p.stderr, "%s: exit %d\n%s" % (tag, p.returncode, p.stderr.decode(errors="replace")[-4000:])
    raw = open(fout, "rb").read()
    lines, nbytes = struct.unpack_from("<2Q", raw, 0)
    assert len(raw) == 16 + nbytes
    o = open(ford, "rb").read()
    K = struct.unpack_from("<I", o, 0)[0]
    assert len(o) == 8 + 8 * K * len(rows) and K == max(1, (order_bits(groups, S, has_sample) + 63) // 64) and K <= words
    w = struct.unpack_from("<%dQ" % (K * len(rows)), o, 8)
    okeys = [sum(w[i * K + k] << (64 * k) for k in range(K)) for i in range(len(rows))]
    return raw[16:], lines, rows, okeys
