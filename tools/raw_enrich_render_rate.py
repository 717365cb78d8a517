"""Time the raw-key enrichment renderer: all 2 x (S + 1) renders of a `barcode-count -e -m` run
(bc_engine_render_raw_enriched over every sample + bc_engine_render_raw_enriched_merged over all of them, for Single and
for Double) into a sink that discards the text.  Workload: that of tools/raw_render_rate.py -- DEL_SCHEME with a sample
file of 4 and NO counted file (three raw 8-base captures), reads made on the device with captures drawn at random, so
nearly every matched read is a row of its own.  Median of `reps` after one warm-up, wall clock around calls that
synchronize by themselves; every rep starts from retired sums (the counts epoch is moved by importing key 0 with
count 0; the first such import, made before anything is counted or timed, leaves a row with count 0 in the map if the
reads did not hold that tuple, later ones add 0 to it: the line counts are asserted to stay what they were), so it pays the raw-key sort and both kinds' project + sort + reduce once and the renders
share them, as one run of the command line does.  The project + sort + reduce part of each kind comes from the engine's
HIP events (bc_engine_raw_enrich_reduce_ms), the raw-key sort's from bc_engine_raw_render_sort_ms.
Prints one JSON line and writes it to profiles/raw_enrich_render_rate.json.
    python tools/raw_enrich_render_rate.py [reads (default 10_500_000)] [reps (default 5)]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [root, os.path.join(root, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ngs_barcode_count_amd as pkg  # noqa: E402

SCHEME = "[8]AGCTACGAATCG{8}TGGA{8}TGGA{8}ACTAGAT"
SAMPLES = ["ACGTACGT", "TTGCAAGC", "GGATCCAA", "CATGTTAG"]
PARTS = [("S", 8), ("C", "AGCTACGAATCG"), ("B", 8), ("C", "TGGA"), ("B", 8), ("C", "TGGA"), ("B", 8), ("C", "ACTAGAT"), ("C", "A")]
R = 60


def make_reads(n, gen):
    """n reads of R bytes on the device: a listed sample barcode, the constants, three captures drawn at random"""
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    samples = torch.tensor([list(s.encode()) for s in SAMPLES], dtype=torch.uint8, device="cuda")
    cols = []
    for kind, v in PARTS:
        if kind == "S":
            cols.append(samples[torch.randint(0, len(SAMPLES), (n,), generator=gen, device="cuda")])
        elif kind == "B":
            cols.append(acgt[torch.randint(0, 4, (n, v), generator=gen, device="cuda")])
        else:
            cols.append(torch.tensor(list(v.encode()), dtype=torch.uint8, device="cuda").expand(n, len(v)))
    out = torch.cat(cols, dim=1).contiguous()
    assert out.shape[1] == R
    return out


def timed(fn, reps):
    fn()  # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_500_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    plan = pkg.Plan(SCHEME)
    for i, s in enumerate(SAMPLES):
        plan.add_sample(s, "Sample_%d" % i)
    plan.set_max_errors(None, None, None)
    assert plan.mode == "sparse"
    eng = pkg.Engine(plan, device=0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    batch = 1 << 21
    for first in range(0, n, batch):
        k = min(batch, n - first)
        reads = make_reads(k, gen)
        torch.cuda.synchronize()
        eng.submit_device(reads.data_ptr(), None, k, R, R)
        eng.sync()
    zero_key = torch.zeros(1, dtype=torch.int64, device="cuda")
    zero_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    counters = eng.counters()
    S = len(SAMPLES)
    lib = eng._lib
    seen = [0, 0]  # bytes, chunks

    def sink(_text, nbytes, _user):
        seen[0] += nbytes
        seen[1] += 1
        return 0

    fn = pkg._lib.TEXT_FN(sink)
    cols = np.arange(S, dtype=np.uint32)
    rows = C.c_uint64()

    def render_kind(kind):
        total = 0
        for s in range(S):
            assert lib.bc_engine_render_raw_enriched(eng._e, kind, s, fn, None, C.byref(rows)) == 0
            total += rows.value
        assert lib.bc_engine_render_raw_enriched_merged(eng._e, kind, cols.ctypes.data, S, fn, None, C.byref(rows)) == 0
        return total, rows.value

    reduce_ms = {pkg.ENRICH_SINGLE: [], pkg.ENRICH_DOUBLE: []}
    sort_ms = []

    def render_all_fresh():
        eng.import_counts(zero_key.data_ptr(), zero_cnt.data_ptr(), 1)  # moves the counts epoch: sums and sort are retired
        before = eng.raw_enrich_reduces()
        for kind in (pkg.ENRICH_SINGLE, pkg.ENRICH_DOUBLE):
            render_kind(kind)
            reduce_ms[kind].append(eng.raw_enrich_reduce_ms())
        assert eng.raw_enrich_reduces() == before + 2
        sort_ms.append(eng.raw_render_sort_ms())

    def render_all_cached():
        for kind in (pkg.ENRICH_SINGLE, pkg.ENRICH_DOUBLE):
            render_kind(kind)

    eng.import_counts(zero_key.data_ptr(), zero_cnt.data_ptr(), 1)  # key 0 is a row from here on, whatever the reads held
    single_lines, single_merged = render_kind(pkg.ENRICH_SINGLE)
    single_bytes = seen[0]
    seen[:] = [0, 0]
    double_lines, double_merged = render_kind(pkg.ENRICH_DOUBLE)
    double_bytes = seen[0]
    t_all, all_fresh = timed(render_all_fresh, reps)
    t_cached, all_cached = timed(render_all_cached, reps)
    # moving the epoch has changed no file: the same lines as before the repetitions
    assert render_kind(pkg.ENRICH_SINGLE) == (single_lines, single_merged)
    assert render_kind(pkg.ENRICH_DOUBLE) == (double_lines, double_merged)
    out = {"tool": "raw_enrich_render_rate", "reads": n, "matched": counters["matched"], "samples": S,
           "single_lines": single_lines, "single_merged_lines": single_merged, "single_text_bytes": single_bytes,
           "double_lines": double_lines, "double_merged_lines": double_merged, "double_text_bytes": double_bytes,
           "device_all_ms": round(t_all, 2), "device_all_ms_all": [round(x, 2) for x in all_fresh],
           "renders_cached_sums_ms": round(t_cached, 2), "renders_cached_sums_ms_all": [round(x, 2) for x in all_cached],
           "single_project_sort_reduce_ms": round(statistics.median(reduce_ms[pkg.ENRICH_SINGLE][1:]), 2),
           "double_project_sort_reduce_ms": round(statistics.median(reduce_ms[pkg.ENRICH_DOUBLE][1:]), 2),
           "single_project_sort_reduce_ms_all": [round(x, 2) for x in reduce_ms[pkg.ENRICH_SINGLE][1:]],
           "double_project_sort_reduce_ms_all": [round(x, 2) for x in reduce_ms[pkg.ENRICH_DOUBLE][1:]],
           "export_rekey_sort_ms": round(statistics.median(sort_ms[1:]), 2),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "raw_enrich_render_rate.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
