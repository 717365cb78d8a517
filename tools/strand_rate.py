"""What the strand setting costs: config-3 shaped synthetic reads resident on the device, ONE submit of 2^25 reads
(argv[1] overrides), timed with HIP events on the engine's stream around submit (+ the wall clock around submit and
sync), one warm submit first, five repetitions, each after a reset that is settled before the clock starts.
  a  forward                                      the default path
  a_traced  forward with a caller's trace on      what recording 9 bytes per read costs the match kernel
  b  both, the same all-forward reads             pass 1 traced + select + one host wait per chunk + a short pass 2
  c  both, the second half of the buffer reversed (bc_strand_orient_device): half of the reads take the second pass
  d  reverse, every read of the buffer reversed   orient(all) + the ordinary launch; counts what (a) counts
b, c and d are reported as ratios to a of the same run.  Per mode the match launches' own HIP-event times (kernel and, in
log mode, fold) are split into first and second pass; `other_ms` is what is left of the submit: select, fix-up, orient
and the host waits.  The orient kernel is also timed alone over the whole buffer, both lines: GB/s read, written and
moved, against the 7.0 TB/s streaming-read ceiling of DESIGN.md.
Prints one JSON line and writes it to profiles/strand_rate.json.
    python tools/strand_rate.py [reads]"""
import json
import os
import statistics
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [root, os.path.join(root, "tests")]
os.environ.setdefault("BC_JIT", "force")
import torch  # noqa: E402

import ngs_barcode_count_amd as pkg  # noqa: E402
import workloads  # noqa: E402

REPS = 5
CEILING_GBPS = 7000.0


def orient_all(stream, src, dst, n, R):
    pkg.orient_device(src[0].data_ptr(), src[1].data_ptr(), R, R, n, dst[0].data_ptr(), dst[1].data_ptr(), stream=stream.cuda_stream)


def measure(mode, bufs, n, R, stream, traced=False):
    w = workloads.make("config3")
    w.plan.set_strand(mode)
    eng = pkg.Engine(w.plan, device=0, stream=stream.cuda_stream)
    trace = None
    if traced:
        trace = (torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda"))
        eng.trace(trace[0].data_ptr(), trace[1].data_ptr())
    submit = lambda: eng.submit_device(bufs[0].data_ptr(), bufs[1].data_ptr(), n, R, R)
    submit()  # warm: compiles / loads the kernels, grows the scratch
    eng.sync()
    ev, wall, first, second = [], [], [], []
    for _ in range(REPS):
        eng.reset()
        eng.sync()
        eng.timing(True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        submit()
        e1.record(stream)
        eng.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(e0.elapsed_time(e1))
        each = eng.kernel_ms_each()
        eng.kernel_ms()
        eng.timing(False)
        # `both` launches pass 1 and pass 2 of a chunk in turn; the others launch once per chunk
        first.append(sum(each[0::2]) if mode == "both" else sum(each))
        second.append(sum(each[1::2]) if mode == "both" else 0.0)
    med = statistics.median(ev)
    i = ev.index(med)
    out = dict(ms=round(med, 3), ms_all=[round(x, 3) for x in ev], wall_ms=round(statistics.median(wall), 3),
               reads_per_s=round(n / (med * 1e-3)), match_first_pass_ms=round(first[i], 3), match_second_pass_ms=round(second[i], 3),
               other_ms=round(med - first[i] - second[i], 3), kernel=eng.kernel_name(), log_folds=eng.count_log_folds(),
               counters=eng.counters(), strand_reads=list(eng.strand_reads()))
    eng.close()
    del trace
    torch.cuda.empty_cache()
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 25
    w = workloads.make("config3")
    R = w.read_len
    stream = torch.cuda.Stream()
    alloc = lambda: (torch.empty(n * R, dtype=torch.uint8, device="cuda"), torch.empty(n * R, dtype=torch.uint8, device="cuda"))
    fwd, rev, mixed = alloc(), alloc(), alloc()
    w.synth.generate_device(0, None, 0, n, fwd[0].data_ptr(), fwd[1].data_ptr())
    torch.cuda.synchronize()
    # the orient kernel alone, both lines of every read
    orient_all(stream, fwd, rev, n, R)
    stream.synchronize()
    oms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        orient_all(stream, fwd, rev, n, R)
        e1.record(stream)
        stream.synchronize()
        oms.append(e0.elapsed_time(e1))
    o_ms = statistics.median(oms)
    line_bytes = 2 * n * R
    half = (n // 2) * R
    for k in (0, 1):
        mixed[k][:half] = fwd[k][:half]
        mixed[k][half:] = rev[k][half:]
    torch.cuda.synchronize()
    res = {"a": measure("forward", fwd, n, R, stream), "a_traced": measure("forward", fwd, n, R, stream, traced=True),
           "b": measure("both", fwd, n, R, stream), "c": measure("both", mixed, n, R, stream), "d": measure("reverse", rev, n, R, stream)}
    a = res["a"]
    assert all(res[k]["counters"]["total_reads"] == n for k in res)
    out = {"tool": "strand_rate", "workload": "config3", "reads": n, "read_len": R, "reps": REPS,
           "strand_chunk": int(os.environ.get("BC_STRAND_CHUNK", 1 << 24)), "modes": res,
           "ratio_to_a": {k: round(res[k]["ms"] / a["ms"], 3) for k in ("a_traced", "b", "c", "d")},
           "same_counters_as_a": {k: res[k]["counters"] == a["counters"] for k in ("a_traced", "b", "c", "d")},
           "orient": {"ms": round(o_ms, 3), "ms_all": [round(x, 3) for x in oms], "read_GBps": round(line_bytes / o_ms / 1e6, 1),
                      "write_GBps": round(line_bytes / o_ms / 1e6, 1), "moved_GBps": round(2 * line_bytes / o_ms / 1e6, 1),
                      "moved_over_streaming_read_ceiling": round(2 * line_bytes / o_ms / 1e6 / CEILING_GBPS, 3),
                      "reads_per_s": round(n / (o_ms * 1e-3))},
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "strand_rate.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
