#!/usr/bin/env python3
"""Ingest rate of the same reads as a BGZF .fastq.gz and as an unaligned .bam, both through bc_fastq_count on one build,
one process.  Writes profiles/bam_ingest_rate.json (and prints the line).

The reads are a 20,000-read DEL file (tests/cases.py, del_mismatch_quality) repeated until the FASTQ text has --mib MiB;
the BAM file holds the same reads (tests/bam_cases.py: names, unmapped flags, no aux), both files BGZF at level 6 with
65,280-byte blocks.  Each is timed as the median of --repeat calls after one warm-up, the files in the page cache,
engine creation excluded.  The two runs must count the same.

    python tools/bam_ingest_rate.py --mib 160
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bam_ingest_rate.py --once --mib 160
    python tools/bam_ingest_rate.py --kernel-stats DIR/.../*_kernel_stats.csv      (adds the kernels' shares to the JSON file)
"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "profiles", "bam_ingest_rate.json")

# the kernels that find the chain of records (candidates, successors, jump pointers, marks, record table); the gather and
# the inflater are counted apart
CHAIN = ("bam_begin_kernel", "bam_count_kernel", "bam_scan_kernel", "bam_positions_kernel", "bam_successor_kernel", "bam_mark_start_kernel",
         "bam_jump_kernel", "bam_mark_kernel", "bam_rec_count_kernel", "bam_rec_table_kernel")


def kernel_shares(path):
    """shares of the device time of a traced --once run, from rocprofv3's kernel_stats.csv"""
    total, groups = 0, {"chain": 0, "gather": 0, "inflate": 0, "match": 0}
    each = {}
    for row in csv.DictReader(open(path)):
        ns, name = int(row["TotalDurationNs"]), row["Name"]
        total += ns
        if any(k + "(" in name for k in CHAIN):
            groups["chain"] += ns
            short = next(k for k in CHAIN if k + "(" in name)
            each[short] = each.get(short, 0) + ns
        elif "bam_gather_kernel(" in name:
            groups["gather"] += ns
        elif "bgzf_inflate_kernel(" in name:
            groups["inflate"] += ns
        elif "match" in name:
            groups["match"] += ns
    out = {"kernel_ns_total": total, "chain_kernels_ns": each}
    for k, v in groups.items():
        out[k + "_share_of_kernel_time"] = v / total if total else 0.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=160)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="the .bam alone, one call after a warm-up, nothing written: the command to put "
                    "behind rocprofv3 --kernel-trace --stats")
    ap.add_argument("--kernel-stats", help="a kernel_stats.csv of a traced --once run: its shares go into the JSON file")
    a = ap.parse_args()
    if a.kernel_stats:
        out = json.load(open(OUT))
        out["traced_once"] = kernel_shares(a.kernel_stats)
        line = json.dumps(out)
        open(OUT, "w").write(line + "\n")
        print(line)
        return
    import bam_cases
    import bgzf
    import cases
    from test_gpu_parity import make_plan
    import ngs_barcode_count_amd as pkg
    c = cases.build_case("del_mismatch_quality", seed=5, n=20000)
    piece = "".join("@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(c["reads"])).encode()
    copies = max(1, (a.mib << 20) // len(piece))
    records, _ = bam_cases.records_text([bam_cases.Rec(name=b"r%d" % i, seq=s, qual=[ord(ch) - 33 for ch in q])
                                         for i, (s, q) in enumerate(c["reads"])])
    plan = make_plan(c)
    out = {"tool": "tools/bam_ingest_rate.py", "reads": copies * len(c["reads"]), "fastq_text_bytes": copies * len(piece),
           "bam_inflated_bytes": len(bam_cases.header()) + copies * len(records), "repeat": a.repeat}
    with tempfile.TemporaryDirectory() as tmp:
        gz, bam = os.path.join(tmp, "a.fastq.gz"), os.path.join(tmp, "a.bam")
        bgzf.write(bam, bam_cases.header() + records * copies)
        if not a.once:
            bgzf.write(gz, piece * copies)
            out["fastq_gz_bytes"] = os.path.getsize(gz)
        out["bam_bytes"] = os.path.getsize(bam)
        seen = {}
        for label, path in (("bam", bam),) if a.once else (("bgzf_fastq", gz), ("bam", bam)):
            times = []
            for k in range((1 if a.once else a.repeat) + 1):
                eng = pkg.Engine(plan, device=0)
                t0 = time.perf_counter()
                total = eng.count_fastq(path)
                eng.sync()
                dt = time.perf_counter() - t0
                got = eng.counters()
                seen[label] = (total, {k2: got[k2] for k2 in got if k2 != "total_reads"}, got["total_reads"])
                eng.close()
                if k:
                    times.append(dt)
            out[label + "_s"] = statistics.median(times)
            out[label + "_s_min_max"] = [min(times), max(times)]
            out[label + "_reads_per_s"] = seen[label][2] / out[label + "_s"]
        if a.once:
            print(json.dumps(out))
            return
        # (the .gz total has the reference's one extra read; the reads counted and their outcomes must agree)
        assert seen["bam"][1:] == seen["bgzf_fastq"][1:] and seen["bam"][0] == out["reads"], "the two runs count differently"
    out["bam_over_bgzf_fastq"] = out["bam_reads_per_s"] / out["bgzf_fastq_reads_per_s"]
    line = json.dumps(out)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
