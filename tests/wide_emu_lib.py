"""Builds and runs tests/emu/wide_emu.cpp: the lane code's wide-key assembly on the host next to a byte-by-byte
restatement of the wave-per-read kernel's key, as a program of its own under AddressSanitizer + UBSan.  TEST-ONLY."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "emu", "wide_emu")
SRCS = [os.path.join(ROOT, "tests", "emu", "wide_emu.cpp"), os.path.join(CSRC, "bc_plan.cpp")]
DEPS = SRCS + [os.path.join(CSRC, h) for h in ("bc_lane.h", "bc_intrin.h", "bc_device_plan.h", "bc_long.h", "bc_plan.hpp")]
KEY_WORDS = 8


def exe():
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", EXE] + SRCS)
    return EXE


def run(scheme, samples, counted, reads, tmp_path, tag="case", budgets=(-1, -1, -1)):
    """-> (key words, outcomes, keys, restated outcomes, restated keys); keys as arrays of n x 8 u64"""
    stride = (max(len(r) for r in reads) + 3) & ~3
    n = len(reads)
    seq = np.full((n, stride), ord("\n"), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint16)
    for i, r in enumerate(reads):
        seq[i, :len(r)] = np.frombuffer(r.encode(), dtype=np.uint8)
        lens[i] = len(r)
    text = lambda s: struct.pack("<I", len(s)) + s.encode()
    fin, fout = (os.path.join(str(tmp_path), tag + e) for e in (".in", ".out"))
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", *budgets) + text(scheme))
        f.write(struct.pack("<I", len(samples or [])) + b"".join(text(s) for s in (samples or [])))
        f.write(struct.pack("<I", len(counted or [])))
        for refs in counted or []:
            f.write(struct.pack("<I", len(refs)) + b"".join(text(s) for s in refs))
        f.write(struct.pack("<2I", n, stride) + seq.tobytes() + lens.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe(), fin, fout], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and not p.stderr, "%s: exit %d\n%s" % (tag, p.returncode, p.stderr.decode(errors="replace")[-4000:])
    raw = open(fout, "rb").read()
    W = struct.unpack_from("<I", raw, 0)[0]
    rec = np.dtype([("oc", "u1"), ("ref_oc", "u1"), ("key", "<u8", KEY_WORDS), ("ref_key", "<u8", KEY_WORDS)])
    assert len(raw) == 4 + n * rec.itemsize
    a = np.frombuffer(raw, dtype=rec, offset=4)
    return W, a["oc"], a["key"], a["ref_oc"], a["ref_key"]
