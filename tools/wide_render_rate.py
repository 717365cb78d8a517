"""Time the wide-key text renderer (bc_engine_render_wide_counts + bc_engine_render_wide_merged, into a sink that
discards the text) against what the file costs on the host path: bc_engine_finish plus one bc_engine_row_text call per
row on the same engine.  Workload: a Barcode-seq scheme with one 40-base capture and nothing known (keys of 3 u64), reads
made on the device with captures drawn at random, so nearly every read is a row of its own.  Each call is timed as the
median of `reps` after one warm-up, wall clock around calls that synchronize by themselves; every rep of the device side
starts from a retired sort (the counts epoch is moved by submitting one read that matches nothing), so it pays export +
order keys + sort + gather once and the two renders share it.  The sort's own device time comes from the engine's HIP
events (bc_engine_wide_render_sort_ms).  The per-row loop is timed over the first `sample_rows` rows and scaled to all of
them (it is one core, linear in the rows; the ctypes call is part of what is timed).
Prints one JSON line and writes it to profiles/wide_render_rate.json.
    python tools/wide_render_rate.py [reads (default 2_000_000)] [reps (default 5)] [sample_rows (default 1_000_000)]"""
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

SCHEME = "GTACCAGTC{40}TGCATGGAC"
PARTS = [("C", "GTACCAGTC"), ("B", 40), ("C", "TGCATGGAC"), ("C", "AC")]
R = 60


def make_reads(n, gen):
    """n reads of R bytes on the device: the constants around a capture drawn at random"""
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    cols = []
    for kind, v in PARTS:
        if kind == "B":
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
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    sample_rows = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
    plan = pkg.Plan(SCHEME)
    assert plan.mode == "sparse"
    eng = pkg.Engine(plan, device=0)
    lib = eng._lib
    assert lib.bc_engine_key_words(eng._e) == 3
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    batch = 1 << 19
    for first in range(0, n, batch):
        k = min(batch, n - first)
        reads = make_reads(k, gen)
        torch.cuda.synchronize()
        eng.submit_device(reads.data_ptr(), None, k, R, R)
        eng.sync()
    nothing = torch.full((R,), ord("A"), dtype=torch.uint8, device="cuda")  # a read without the constants
    counters = eng.counters()
    seen = [0, 0]  # bytes, chunks

    def sink(_text, nbytes, _user):
        seen[0] += nbytes
        seen[1] += 1
        return 0

    fn = pkg._lib.TEXT_FN(sink)
    cols = np.zeros(1, dtype=np.uint32)
    rows = C.c_uint64()

    def render_counts():
        assert lib.bc_engine_render_wide_counts(eng._e, 0, fn, None, C.byref(rows)) == 0
        return rows.value

    def render_merged():
        assert lib.bc_engine_render_wide_merged(eng._e, cols.ctypes.data, 1, fn, None, C.byref(rows)) == 0
        return rows.value

    sort_ms = []

    def render_all_fresh():
        eng.submit_device(nothing.data_ptr(), None, 1, R, R)  # moves the counts epoch: the next render sorts anew
        eng.sync()
        before = eng.wide_render_sorts()
        render_counts()
        render_merged()
        assert eng.wide_render_sorts() == before + 1
        sort_ms.append(eng.wide_render_sort_ms())

    n_rows = eng.finish()
    assert render_counts() == n_rows, "the file holds every row finish() hands out"
    counts_bytes = seen[0]
    t_counts, _ = timed(render_counts, reps)   # (the sort is cached: the render alone)
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
    out = {"tool": "wide_render_rate", "reads": n, "matched": counters["matched"], "rows": n_rows, "key_words": 3,
           "counts_text_bytes": counts_bytes,
           "render_counts_cached_sort_ms": round(t_counts, 2), "render_merged_cached_sort_ms": round(t_merged, 2),
           "device_all_ms": round(t_all, 2), "device_all_ms_all": [round(x, 2) for x in all_render],
           "export_order_sort_gather_ms": round(t_sort, 2), "finish_ms": round(t_finish, 2),
           "finish_ms_all": [round(x, 2) for x in all_finish], "row_text_us_per_row": round(us_per_row, 3),
           "row_text_rows_timed": k, "host_rows_ms_scaled": round(host_ms, 1), "host_over_device": round(host_ms / t_all, 1),
           "sort_Mrows_per_s": round(n_rows / (t_sort * 1e-3) / 1e6, 1) if t_sort else None,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "wide_render_rate.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
