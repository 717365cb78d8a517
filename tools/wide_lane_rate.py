"""reads/s of ONE wide-key plan on the two match kernels: Barcode-seq with a 30-base lineage barcode and no conversion
file, GTACCAGTC{30}TGCATGGAC, 100-base device-resident reads whose captures are drawn from 50,000 barcodes.
  lane:      this build with BC_WIDE_LANE=1 -- the lane-per-read kernel assembles the wide key (specialised kernel,
             BC_JIT=force)
  baseline:  a library built from the PARENT commit, given as BC_LIB=<file> (the wave-per-read kernel, the only one that
             ran such a plan before) -- not this build with the switch off
4,000,000 reads (argv[1] overrides).  Each engine counts the batch once to warm its kernel (and compile it), then five
timed repetitions, each after a reset that is not timed: wall clock around submit + sync, and the kernel's own time from
the engine's HIP events.  The median of the five is the figure.  Both engines must end with the same counters and rows.
Prints one JSON line and writes it to profiles/wide_lane_rate.json.
    BC_LIB=<parent build>/libbarcode_count_hip.so python tools/wide_lane_rate.py [reads]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [root, os.path.join(root, "tests")]
BASELINE = os.environ.pop("BC_LIB", None)  # (the package itself loads this build)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ngs_barcode_count_amd as pkg  # noqa: E402
from ngs_barcode_count_amd import _lib  # noqa: E402

SCHEME = "GTACCAGTC{30}TGCATGGAC"
R, CAP, REPS = 100, 30, 5


def make_reads(n):
    rng = np.random.default_rng(1)
    pool = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (50_000, CAP))]
    reads = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, R))].copy()
    pick = rng.integers(0, len(pool), n)
    off = rng.integers(0, R - (CAP + 18) - 1, n)
    a, b = np.frombuffer(b"GTACCAGTC", dtype=np.uint8), np.frombuffer(b"TGCATGGAC", dtype=np.uint8)
    idx = np.arange(n)
    for k in range(9):
        reads[idx, off + k] = a[k]
        reads[idx, off + 9 + CAP + k] = b[k]
    for k in range(CAP):
        reads[idx, off + 9 + k] = pool[pick, k]
    return reads


def load_older(path):
    """a library of an earlier commit: the functions it has, declared as this build declares them"""
    lib = C.CDLL(os.path.abspath(path))
    for api in (_lib.PLAN_API, _lib.ENGINE_API):
        for name, (res, args) in api.items():
            if hasattr(lib, name):
                f = getattr(lib, name)
                f.restype, f.argtypes = res, args
    return lib


def measure(lib, switch, d, n):
    os.environ["BC_WIDE_LANE"] = switch
    os.environ["BC_JIT"] = "force"
    plan = pkg.Plan(SCHEME, lib=lib) if lib is not None else pkg.Plan(SCHEME)
    eng = pkg.Engine(plan, device=0)
    eng.submit_device(d.data_ptr(), None, n, R, R)  # warm-up: compiles / loads the kernel, grows the table
    eng.sync()
    wall, kern = [], []
    for _ in range(REPS):
        eng.reset()
        eng.sync()
        eng.timing(True)
        t0 = time.perf_counter()
        eng.submit_device(d.data_ptr(), None, n, R, R)
        eng.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(eng.kernel_ms()[0])
        eng.timing(False)
    out = dict(kernel=eng.kernel_name(), wall_ms=round(statistics.median(wall), 3), wall_ms_all=[round(x, 3) for x in wall],
               kernel_ms=round(statistics.median(kern), 3), kernel_ms_all=[round(x, 3) for x in kern],
               reads_per_s=round(n / (statistics.median(wall) * 1e-3)), counters=eng.counters(), rows=eng.finish())
    rows = eng.result_rows()
    eng.close()
    return out, rows


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
    if not BASELINE:
        sys.exit("BC_LIB=<library built from the parent commit> is required: the baseline is that build")
    d = torch.from_numpy(make_reads(n).reshape(-1)).cuda()
    torch.cuda.synchronize()
    lane, lane_rows = measure(None, "1", d, n)
    base, base_rows = measure(load_older(BASELINE), "0", d, n)
    assert "match_count" in lane["kernel"] and base["kernel"] == "long_match_kernel", (lane["kernel"], base["kernel"])
    assert lane["counters"] == base["counters"] and lane_rows == base_rows
    out = {"tool": "wide_lane_rate", "scheme": SCHEME, "reads": n, "read_len": R, "reps": REPS,
           "lane": lane, "baseline_parent_build": base,
           "lane_over_baseline": round(lane["reads_per_s"] / base["reads_per_s"], 2), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "wide_lane_rate.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
