#!/usr/bin/env python3
"""Ingest rate of one FASTQ text as plain text, as BGZF inflated on the device, and as the same BGZF file through zlib
on the host (BC_GZ_DEVICE=0: the path every .gz took before the device inflater).  One process, one JSON line.

The text is a 20,000-read DEL file (tests/cases.py, del_mismatch_quality) repeated to --mib MiB, written as BGZF at
level 6 with 65,280-byte blocks; each variant is timed as the median of --repeat bc_fastq_count calls after one warm-up,
the files in the page cache, engine creation excluded.  The counts of the two BGZF runs must agree.

    python tools/gz_ingest_rate.py --mib 160 > profiles/bgzf_ingest_rate.json
    python tools/gz_ingest_rate.py --gzip --mib 160                  (ordinary gzip; writes profiles/gzip_ingest_rate.json)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/gz_ingest_rate.py --gzip --once --mib 160
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
    ap.add_argument("--gzip", action="store_true", help="an ordinary gzip -6 file through zlib (BC_GZ_DEVICE=1) and through the "
                    "device's span inflater (BC_GZ_DEVICE=all); writes profiles/gzip_ingest_rate.json")
    ap.add_argument("--once", action="store_true", help="with --gzip: the device path alone, one call after a warm-up, nothing "
                    "written: the command to put behind rocprofv3 --kernel-trace --stats (profiles/gzip_kernel_stats.csv)")
    a = ap.parse_args()
    if a.gzip:
        return gzip_mode(a)
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


def gzip_mode(a):
    """the same text written by gzip -6 (Python's gzip module): zlib on the host, the path such a file takes by default and
    the only fair yardstick, against the span inflater; median of --repeat after a warm-up, same file, same call"""
    import gzip
    import re
    import subprocess
    import cases
    from test_gpu_parity import make_plan
    import ngs_barcode_count_amd as pkg
    c = cases.build_case("del_mismatch_quality", seed=5, n=20000)
    piece = "".join("@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(c["reads"])).encode()
    text = piece * max(1, (a.mib << 20) // len(piece))
    plan = make_plan(c)
    out = {"tool": "tools/gz_ingest_rate.py --gzip", "text_bytes": len(text), "repeat": a.repeat}
    with tempfile.TemporaryDirectory() as tmp:
        gz = os.path.join(tmp, "a.fastq.gz")
        with gzip.GzipFile(gz, "wb", compresslevel=6) as f:
            f.write(text)
        out["gz_bytes"] = os.path.getsize(gz)
        if a.once:
            a.repeat = 1
        seen = {}
        for label, dev in (("device", "all"),) if a.once else (("zlib", "1"), ("device", "all")):
            os.environ["BC_GZ_DEVICE"] = dev
            times = []
            for k in range(a.repeat + 1):
                eng = pkg.Engine(plan, device=0)
                t0 = time.perf_counter()
                total = eng.count_fastq(gz)
                eng.sync()
                dt = time.perf_counter() - t0
                seen[label] = (total, eng.counters(), eng.gz_segments_inflated())
                eng.close()
                if k:
                    times.append(dt)
            out[label + "_s"] = statistics.median(times)
            out[label + "_s_min_max"] = [min(times), max(times)]
            out[label + "_reads_per_s"] = total / out[label + "_s"]
        out["segments"] = seen["device"][2]
        if a.once:
            out["calls_traced"] = 2
            print(json.dumps(out))
            return
        assert seen["device"][:2] == seen["zlib"][:2], "the two runs count differently"
        # spans, rejected candidates and retries are what BC_INGEST_VERBOSE reports: one more call, in a child process
        env = dict(os.environ, BC_GZ_DEVICE="all", BC_INGEST_VERBOSE="1")
        code = ("import sys; sys.path[:0] = %r; import cases, ngs_barcode_count_amd as pkg; from test_gpu_parity import make_plan; "
                "c = cases.build_case('del_mismatch_quality', seed=5, n=20000); e = pkg.Engine(make_plan(c), device=0); "
                "e.count_fastq(%r); e.close()" % ([ROOT, os.path.join(ROOT, "tests")], gz))
        err = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True).stderr
        m = re.search(r"(\d+) spans, (\d+) segments, (\d+) candidates rejected, (\d+) retries", err)
        if m:
            out["spans"], out["rejected_candidates"], out["retries"] = int(m.group(1)), int(m.group(3)), int(m.group(4))
            out["segments_per_span"] = int(m.group(2)) / max(1, int(m.group(1)))
    out["device_over_zlib"] = out["device_reads_per_s"] / out["zlib_reads_per_s"]
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "gzip_ingest_rate.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
