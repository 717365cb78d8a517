#!/usr/bin/env python3
"""Ingest rate of one FASTQ text as plain text, as BGZF inflated on the device, and as the same BGZF file through zlib
on the host (BC_GZ_DEVICE=0: the path every .gz took before the device inflater).  One process, one JSON line.

The text is a 20,000-read DEL file (tests/cases.py, del_mismatch_quality) repeated to --mib MiB, written as BGZF at
level 6 with 65,280-byte blocks; each variant is timed as the median of --repeat bc_fastq_count calls after one warm-up,
the files in the page cache, engine creation excluded.  The counts of the two BGZF runs must agree.

    python tools/gz_ingest_rate.py --mib 160 > profiles/bgzf_ingest_rate.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=160)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import bgzf
    import cases
    from test_gpu_parity import make_plan
    import ngs_barcode_count_amd as pkg
    c = cases.build_case("del_mismatch_quality", seed=5, n=20000)
    piece = "".join("@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(c["reads"])).encode()
    text = piece * max(1, (a.mib << 20) // len(piece))
    plan = make_plan(c)
    out = {"tool": "tools/gz_ingest_rate.py", "text_bytes": len(text)}
    with tempfile.TemporaryDirectory() as tmp:
        plain, gz = os.path.join(tmp, "a.fastq"), os.path.join(tmp, "a.fastq.gz")
        open(plain, "wb").write(text)
        bgzf.write(gz, text)
        out["gz_bytes"] = os.path.getsize(gz)
        out["compressed_over_inflated"] = out["gz_bytes"] / len(text)
        seen = {}
        for label, path, dev in (("plain", plain, "1"), ("bgzf_device", gz, "1"), ("bgzf_zlib", gz, "0")):
            os.environ["BC_GZ_DEVICE"] = dev
            times = []
            for k in range(a.repeat + 1):
                eng = pkg.Engine(plan, device=0)
                t0 = time.perf_counter()
                total = eng.count_fastq(path)
                eng.sync()
                dt = time.perf_counter() - t0
                seen[label] = (total, eng.counters(), eng.gz_blocks_inflated())
                eng.close()
                if k:
                    times.append(dt)
            out[label + "_s"] = statistics.median(times)
            out[label + "_reads_per_s"] = total / out[label + "_s"]
        assert seen["bgzf_device"][:2] == seen["bgzf_zlib"][:2], "the two BGZF runs count differently"
        out["bgzf_blocks"] = seen["bgzf_device"][2]
    out["device_over_zlib"] = out["bgzf_device_reads_per_s"] / out["bgzf_zlib_reads_per_s"]
    out["device_over_plain"] = out["bgzf_device_reads_per_s"] / out["plain_reads_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
