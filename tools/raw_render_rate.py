"""Time the raw-key text renderer (bc_engine_render_raw_counts over every sample + bc_engine_render_raw_merged over all
of them, into a sink that discards the text) against what the files cost on the host path: bc_engine_finish plus one
bc_engine_row_text call per row on the same engine.  Workload: DEL_SCHEME with a sample file of 4 and NO counted file
(three raw 8-base captures), reads made on the device with captures drawn at random, so nearly every matched read is a
row of its own.  Each call is timed as the median of `reps` after one warm-up, wall clock around calls that synchronize
by themselves; every rep of the device side starts from a retired sort (the counts epoch is moved by importing one
key with count 0, which adds nothing), so it pays export + re-key + sort once and the S + 1 renders share it, as one `barcode-count -m` run does.  The sort's own device time comes from the
engine's HIP events (bc_engine_raw_render_sort_ms).  The per-row loop is timed over the first `sample_rows` rows and
scaled to all of them (it is one core, linear in the rows; the ctypes call is part of what is timed).
Prints one JSON line and writes it to profiles/raw_render_rate.json.
    python tools/raw_render_rate.py [reads (default 10_500_000)] [reps (default 5)] [sample_rows (default 1_000_000)]"""
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
    sample_rows = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
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

    def render_counts():
        total = 0
        for s in range(S):
            assert lib.bc_engine_render_raw_counts(eng._e, s, fn, None, C.byref(rows)) == 0
            total += rows.value
        return total

    def render_merged():
        assert lib.bc_engine_render_raw_merged(eng._e, cols.ctypes.data, S, fn, None, C.byref(rows)) == 0
        return rows.value

    sort_ms = []

    def render_all_fresh():
        eng.import_counts(zero_key.data_ptr(), zero_cnt.data_ptr(), 1)  # moves the counts epoch: the next render sorts anew
        before = eng.raw_render_sorts()
        render_counts()
        render_merged()
        assert eng.raw_render_sorts() == before + 1
        sort_ms.append(eng.raw_render_sort_ms())

    n_rows = eng.finish()
    assert render_counts() == n_rows, "the per-sample files hold every row finish() hands out"
    counts_bytes = seen[0]
    seen[:] = [0, 0]
    merged_rows = render_merged()
    merged_bytes = seen[0]
    t_counts, _ = timed(render_counts, reps)   # (the sort is cached: the renders alone)
    t_merged, _ = timed(render_merged, reps)
    t_all, all_render = timed(render_all_fresh, reps)
    t_sort = statistics.median(sort_ms[1:])
    t_finish, all_finish = timed(lambda: eng.finish(), reps)
    k = min(sample_rows, n_rows)
    sb, tb, cnt = C.create_string_buffer(64), C.create_string_buffer(2048), C.c_uint64()
    t0 = time.perf_counter()
    for i in range(k):
        lib.bc_engine_row_text(eng._e, i, sb, 64, tb, 2048, C.byref(cnt))
    us_per_row = (time.perf_counter() - t0) * 1e6 / max(k, 1)
    host_ms = t_finish + us_per_row * n_rows * 1e-3
    out = {"tool": "raw_render_rate", "reads": n, "matched": counters["matched"], "rows": n_rows, "merged_rows": merged_rows,
           "counts_text_bytes": counts_bytes, "merged_text_bytes": merged_bytes,
           "render_counts_cached_sort_ms": round(t_counts, 2), "render_merged_cached_sort_ms": round(t_merged, 2),
           "device_all_ms": round(t_all, 2), "device_all_ms_all": [round(x, 2) for x in all_render],
           "export_rekey_sort_ms": round(t_sort, 2), "finish_ms": round(t_finish, 2),
           "finish_ms_all": [round(x, 2) for x in all_finish], "row_text_us_per_row": round(us_per_row, 3),
           "row_text_rows_timed": k, "host_rows_ms_scaled": round(host_ms, 1), "host_over_device": round(host_ms / t_all, 1),
           "sort_Mpairs_per_s": round(n_rows / (t_sort * 1e-3) / 1e6, 1) if t_sort else None,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "raw_render_rate.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
