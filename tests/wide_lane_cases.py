"""Wide-key plans the lane-per-read kernel can run (BC_WIDE_LANE=1; csrc/bc_plan.cpp lower(allow_wide)), for
tests/test_wide_lane_emulation.py (the lane code on the host) and tests/test_gpu_wide_lane.py (the kernel).  The case
format, the read generator and three of the cases are tests/test_gpu_wide_keys.py's."""
import numpy as np

import oracle_lib
import test_gpu_wide_keys as twk

SCHEMES = {
    # one 28-base raw capture: 84 payload bits, the N plane crosses from word 1 into word 2
    "raw_28": dict(scheme="GTACCAGTC{28}TGCATGGAC", parts=[("const", "GTACCAGTC"), ("cap", 28, 0), ("const", "TGCATGGAC")],
                   pools=[(300, 28)]),
    # one 32-base raw capture: plane fields of 32 bits, at bits 0, 32 and 64
    "raw_32": dict(scheme="GTACCAGTC{32}TGCATGGAC", parts=[("const", "GTACCAGTC"), ("cap", 32, 0), ("const", "TGCATGGAC")],
                   pools=[(300, 32)]),
    # 22 + 21 raw bases: each fits the 64-bit key, together they do not; the second capture's fields start at bit 66
    "raw_22_21": dict(scheme="CCTAGG{22}AATT{21}GGATCC", parts=[("const", "CCTAGG"), ("cap", 22, 0), ("const", "AATT"), ("cap", 21, 1), ("const", "GGATCC")],
                      pools=[(30, 22), (40, 21)]),
    "three_raw_20": twk.CASES["three_raw_20"],                  # 180 payload bits
    "known_plus_random_30": twk.CASES["known_plus_random_30"],  # an 8-base sample set, an 8-base counted set, 30 random
    # a 20-base counted set of 100 references (hash + search) and a 32-base random barcode
    "set_20_plus_random_32": dict(scheme="CCTAGG{20}AATT(32)GGATCC", parts=[("const", "CCTAGG"), ("cap", 20, 0), ("const", "AATT"), ("cap", 32, 1), ("const", "GGATCC")],
                                  pools=[(100, 20), (400, 32)], counted_from=[0]),
    "raw_plus_random_28": twk.CASES["raw_plus_random_28"],      # a 24-base raw capture and a 28-base random barcode
}


def pools_and_reads(name, n, seed, **kw):
    c = SCHEMES[name]
    rng = np.random.default_rng(seed + 1000)
    pools = [twk._pool(rng, k, ln) for k, ln in c["pools"]]
    return c, pools, twk._reads(c["parts"], n, seed, pools, **kw)


def sets_of(c, pools):
    samples = {s: "sample_%d" % i for i, s in enumerate(pools[c["samples_from"]])} if "samples_from" in c else None
    counted = [pools[k] for k in c["counted_from"]] if "counted_from" in c else None
    return samples, counted


def oracle_of(c, pools):
    samples, counted = sets_of(c, pools)
    return oracle_lib.Oracle(c["scheme"], samples=samples, counted=counted)


def plan_of(c, pools, lib=None):
    import ngs_barcode_count_amd as pkg
    plan = pkg.Plan(c["scheme"], lib=lib) if lib is not None else pkg.Plan(c["scheme"])
    samples, counted = sets_of(c, pools)
    for s, i in (samples or {}).items():
        plan.add_sample(s, i)
    for b, refs in enumerate(counted or []):
        for s in refs:
            plan.add_counted(b, s, s)
    return plan
