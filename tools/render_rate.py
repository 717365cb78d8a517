"""Time the device text renderer (bc_engine_render_counts over every sample + bc_engine_render_merged over all of them,
into a sink that discards the text) against bc_engine_finish on the same engine: synthetic config-3 reads (BASELINE
sizes: 4 samples x 1000^3 tuples, a 16 GB table) counted on the device, then each call timed as the median of `reps`
after one warm-up, wall clock around calls that synchronize by themselves.  Prints one JSON line and writes it to
profiles/render_rate.json.
    python tools/render_rate.py [reads (default 100_000_000)] [reps (default 5)]"""
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
import workloads  # noqa: E402


def timed(fn, reps):
    fn()  # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    w = workloads.make("config3")
    R = w.read_len
    eng = pkg.Engine(w.plan, device=0)
    batch = 1 << 24
    dseq = torch.empty(batch * R, dtype=torch.uint8, device="cuda")
    dqual = torch.empty(batch * R, dtype=torch.uint8, device="cuda")
    for first in range(0, n, batch):
        k = min(batch, n - first)
        w.synth.generate_device(0, None, first, k, dseq.data_ptr(), dqual.data_ptr())
        torch.cuda.synchronize()
        eng.submit_device(dseq.data_ptr(), dqual.data_ptr() if w.min_quality > 0 else None, k, R, R)
        eng.sync()
    del dseq, dqual
    counters = eng.counters()
    S = len(w.plan.samples())
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
            assert lib.bc_engine_render_counts(eng._e, s, fn, None, C.byref(rows)) == 0
            total += rows.value
        return total

    def render_merged():
        assert lib.bc_engine_render_merged(eng._e, cols.ctypes.data, S, fn, None, C.byref(rows)) == 0
        return rows.value

    def render_all():
        render_counts()
        render_merged()

    n_rows = eng.finish()
    assert render_counts() == n_rows, "the per-sample files hold every row finish() hands out"
    counts_bytes = seen[0]
    seen[:] = [0, 0]
    merged_rows = render_merged()
    merged_bytes = seen[0]
    t_counts, _ = timed(render_counts, reps)
    t_merged, _ = timed(render_merged, reps)
    t_all, all_render = timed(render_all, reps)
    t_finish, all_finish = timed(lambda: eng.finish(), reps)
    table_bytes = eng.table_entries * 4
    out = {"tool": "render_rate", "reads": n, "matched": counters["matched"], "table_entries": eng.table_entries,
           "rows": n_rows, "merged_rows": merged_rows, "counts_text_bytes": counts_bytes, "merged_text_bytes": merged_bytes,
           "render_counts_ms": round(t_counts, 2), "render_merged_ms": round(t_merged, 2), "render_all_ms": round(t_all, 2),
           "finish_ms": round(t_finish, 2), "render_all_ms_all": [round(x, 2) for x in all_render],
           "finish_ms_all": [round(x, 2) for x in all_finish],
           # every render sweeps its part of the table twice (sizes, then text): counts + merged = 4 sweeps of the table
           "table_sweep_GBps": round(4 * table_bytes / (t_all * 1e-3) / 1e9, 1),
           "text_GBps": round((counts_bytes + merged_bytes) / (t_all * 1e-3) / 1e9, 2),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "render_rate.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
