"""Time the device enrichment renderer (bc_engine_render_enriched for Single and Double over every sample, and both
bc_engine_render_enriched_merged over all of them, into a sink that discards the text) against bc_engine_enrich + its
host copy on the same engine: synthetic config-3 reads (BASELINE sizes: 4 samples x 1000^3 tuples, a 16 GB table)
counted on the device.  The first run of every render is timed on its own -- it holds the one pass over the table that
computes the sums --, then each call as the median of `reps` after that warm-up, wall clock around calls that
synchronize by themselves.  Prints one JSON line and writes it to profiles/enrich_render_rate.json.
    python tools/enrich_render_rate.py [reads (default 100_000_000)] [reps (default 5)] [output file]"""
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


def once(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def timed(fn, reps):
    out = [once(fn) for _ in range(reps)]
    return statistics.median(out), out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dest = sys.argv[3] if len(sys.argv) > 3 else os.path.join(root, "profiles", "enrich_render_rate.json")
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
    kinds = (pkg.ENRICH_SINGLE, pkg.ENRICH_DOUBLE)

    def render_samples():
        total = 0
        for kind in kinds:
            for s in range(S):
                assert lib.bc_engine_render_enriched(eng._e, kind, s, fn, None, C.byref(rows)) == 0
                total += rows.value
        return total

    def render_merged():
        total = 0
        for kind in kinds:
            assert lib.bc_engine_render_enriched_merged(eng._e, kind, cols.ctypes.data, S, fn, None, C.byref(rows)) == 0
            total += rows.value
        return total

    def render_all():
        render_samples()
        render_merged()

    t_first = once(render_all)  # the table pass, the fold (none here: no shared IDs), the label pool, and the text
    seen[:] = [0, 0]
    sample_lines = render_samples()
    sample_bytes = seen[0]
    seen[:] = [0, 0]
    merged_lines = render_merged()
    merged_bytes = seen[0]
    t_samples, _ = timed(render_samples, reps)
    t_merged, _ = timed(render_merged, reps)
    t_all, all_render = timed(render_all, reps)
    eng.enrichment()  # warm-up
    t_enrich, all_enrich = timed(lambda: eng.enrichment(), reps)  # bc_engine_enrich + the copy of its sums to the host
    out = {"tool": "enrich_render_rate", "reads": n, "matched": counters["matched"], "table_entries": eng.table_entries,
           "sample_lines": sample_lines, "merged_lines": merged_lines, "sample_text_bytes": sample_bytes,
           "merged_text_bytes": merged_bytes, "first_render_all_ms": round(t_first, 2),
           "render_samples_ms": round(t_samples, 2), "render_merged_ms": round(t_merged, 2), "render_all_ms": round(t_all, 2),
           "enrich_and_copy_ms": round(t_enrich, 2), "render_all_ms_all": [round(x, 2) for x in all_render],
           "enrich_and_copy_ms_all": [round(x, 2) for x in all_enrich],
           "text_GBps": round((sample_bytes + merged_bytes) / (t_all * 1e-3) / 1e9, 2),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    with open(dest, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
