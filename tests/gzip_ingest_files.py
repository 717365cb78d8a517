"""The .fastq.gz files of the gzip-device ingest tests (test_gpu_gzip_ingest.py, test_gpu_cli_gzip.py): about 20,000
reads of a small DEL scheme, written the ways gzip, pigz and a converter write them.  TEST-ONLY."""
import functools
import os
import random

import cases
import gunzip_cases

# (BC_INGEST_CHUNK bounds the zlib run's chunks; the gzip-device path never runs with a text buffer below 1 MiB, since a
# deflate block's text has to fit it, so its run cuts this 4.5 MB text into chunks of 1 MiB: records still straddle them)
ENV = {"BC_INGEST_CHUNK": "65536", "BC_GZ_SPAN_BYTES": "8192", "BC_GZ_PART_BYTES": "1024"}
N_READS = 20000


@functools.lru_cache(maxsize=None)
def case():
    return cases.build_case("del_mismatch_quality", seed=83, n=N_READS)


@functools.lru_cache(maxsize=None)
def text():
    rng = random.Random(5)
    return "".join("@M01:%d:%d %d:N:0\n%s\n+\n%s\n" % (i, rng.randint(1000, 29999), i % 3, s, q)
                   for i, (s, q) in enumerate(case()["reads"])).encode()


@functools.lru_cache(maxsize=None)
def variants():
    """name -> the file's bytes"""
    t = text()
    half = t.index(b"\n@M01:", len(t) // 2) + 1
    seq = t.split(b"\n")[1]
    out = {"level_%d" % lv: gunzip_cases.gzip_member(t, lv) for lv in (1, 6, 9)}
    out["two_members"] = gunzip_cases.gzip_member(t[:half], 6) + gunzip_cases.gzip_member(t[half:], 6)
    out["fname_fextra"] = gunzip_cases.gzip_member(t, 6, name=b"reads.fastq", extra=b"XY\x03\x00abc")
    out["no_final_newline"] = gunzip_cases.gzip_member(t[:-1], 6)
    out["three_lines_into_a_record"] = gunzip_cases.gzip_member(t + b"@tail\n" + seq + b"\n+\n", 6)
    return out


def write(tmp, name, blob):
    path = os.path.join(str(tmp), name + ".fastq.gz")
    with open(path, "wb") as f:
        f.write(blob)
    return path
