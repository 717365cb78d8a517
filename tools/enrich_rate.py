"""Time bc_engine_enrich against bc_engine_finish on the same engine: synthetic config-3 reads (BASELINE sizes:
4 samples x 1000^3 tuples, a 16 GB table) counted on the device, then each call timed as the median of `reps` after one
warm-up, wall clock around calls that synchronize by themselves.  Prints one JSON line.
    python tools/enrich_rate.py [reads (default 100_000_000)] [reps (default 5)]"""
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
    counters = eng.counters()
    nonzero = eng.nonzero_entries()
    singles, doubles = eng.enrichment()
    total = int(singles[0].sum())
    assert total == counters["matched"], (total, counters["matched"])
    s, b, c = eng.rows()  # one cross-check of the device sums against the rows (group 2, every sample)
    exp = torch.zeros(singles[2].shape, dtype=torch.int64)
    exp.index_put_((torch.from_numpy(s.astype("int64")), torch.from_numpy(b[:, 2].astype("int64"))),
                   torch.from_numpy(c.astype("int64")), accumulate=True)
    assert (exp.numpy().astype("uint64") == singles[2]).all()
    del s, b, c, exp
    lib = eng._lib
    ptr = lambda a: a.ctypes.data
    buf_s = np.zeros(sum(a.size for a in singles), dtype=np.uint64)
    buf_d = np.zeros(sum(a.size for a in doubles.values()), dtype=np.uint64)

    def enrich():
        assert lib.bc_engine_enrich(eng._e, ptr(buf_s), ptr(buf_d)) == 0

    def enrich_singles():
        assert lib.bc_engine_enrich(eng._e, ptr(buf_s), None) == 0

    def finish():
        eng.finish()

    t_enrich, all_enrich = timed(enrich, reps)
    t_single, _ = timed(enrich_singles, reps)
    t_finish, all_finish = timed(finish, reps)
    print(json.dumps({"tool": "enrich_rate", "reads": n, "matched": counters["matched"], "table_entries": eng.table_entries,
                      "nonzero_entries": nonzero, "single_entries": int(buf_s.size), "double_entries": int(buf_d.size),
                      "enrich_ms": round(t_enrich, 2), "enrich_singles_only_ms": round(t_single, 2),
                      "finish_ms": round(t_finish, 2), "enrich_ms_all": [round(x, 2) for x in all_enrich],
                      "finish_ms_all": [round(x, 2) for x in all_finish], "device": torch.cuda.get_device_name(0)}))
    eng.close()


if __name__ == "__main__":
    main()
