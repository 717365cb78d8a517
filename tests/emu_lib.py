"""Builds and binds tests/emu/libbc_emu.so: the host emulation of the kernel's lane code
(csrc/bc_lane.h) plus the host-only plan code (csrc/bc_plan.cpp).  TEST-ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
SO = os.path.join(ROOT, "tests", "emu", "libbc_emu.so")
# "static": the lane code compiled with the counting form of the scheme-specialised kernels (carry-save accumulation of
# directly extracted windows, bc_lane.h count_mismatches_static), which otherwise only a GPU build would exercise
VARIANTS = {"generic": (SO, []), "static": (SO.replace(".so", "_static.so"), ["-DBC_EMU_STATIC_COUNT=1"])}
SRCS = [os.path.join(ROOT, "tests", "emu", "emu.cpp"), os.path.join(CSRC, "bc_plan.cpp")]
DEPS = SRCS + [os.path.join(CSRC, f) for f in ("bc_lane.h", "bc_intrin.h", "bc_device_plan.h", "bc_plan.hpp")]

_libs = {}


def lib(variant="generic"):
    if variant not in _libs:
        so, flags = VARIANTS[variant]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in DEPS):
            subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fPIC", "-shared",
                                   "-pthread", "-o", so] + flags + SRCS)
        import ngs_barcode_count_amd as pkg
        L = C.CDLL(so)
        pkg._lib.declare(L, pkg._lib.PLAN_API)
        L.emu_plan_create.restype = C.c_void_p
        L.emu_plan_create.argtypes = [C.c_void_p]
        L.emu_plan_lower.restype = C.c_void_p
        L.emu_plan_lower.argtypes = [C.c_void_p]
        L.emu_plan_destroy.argtypes = [C.c_void_p]
        L.emu_table_entries.restype = C.c_uint64
        L.emu_table_entries.argtypes = [C.c_void_p]
        L.emu_discard_counts.argtypes = [C.c_void_p]
        L.emu_process.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_process2.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_group_layout.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_rspace.restype = C.c_uint64
        L.emu_rspace.argtypes = [C.c_void_p]
        _libs[variant] = L
    return _libs[variant]


def make_plan(case, variant="generic"):
    """Plan (host-only functions, served by the emu library) for a cases.build_case() dict"""
    import ngs_barcode_count_amd as pkg
    p = pkg.Plan(case["scheme"], lib=lib(variant))
    if case.get("samples"):
        for s, i in case["samples"].items():
            p.add_sample(s, i)
    if case.get("counted"):
        for bi, refs in enumerate(case["counted"]):
            for r in refs:
                p.add_counted(bi, r, r)
    kw = case.get("kwargs", {})
    p.set_max_errors(kw.get("max_sample"), kw.get("max_barcode"), kw.get("max_constant"))
    p.set_min_quality(kw.get("min_quality", 0.0))
    return p


def open_plan(plan):
    """the emulation's lowered form of `plan`, for several emulate(handle=) calls; close_plan() frees it"""
    L = plan._lib
    e = L.emu_plan_create(plan._p)
    if not e:
        raise RuntimeError(L.bc_last_error().decode())
    return e


def close_plan(plan, handle):
    plan._lib.emu_plan_destroy(handle)


LAYOUT_FIELDS = ("mode", "seed_nb", "seed_blen", "seed2_nb", "seed2_blen", "seed3_nb", "seed3_blen", "tier_blen",
                 "tier_stride", "tier_compact", "n_idx", "n_odd", "lhash_nb", "lhash_complete", "len", "n_refs", "max_err",
                 "defer_search")
LAYOUT_ARRAYS = ("seed_off", "seed_list", "seed2_off", "seed2_list", "seed3_off", "seed3_list", "tier_off", "tier_list",
                 "tier_bkt", "odd_list", "r1", "r2")


def group_layout(plan, group=0, handle=None):
    """what bc_plan::lower chose for one group: {field: int} for LAYOUT_FIELDS (defer_search is the plan's) plus copies
    of the index arrays of LAYOUT_ARRAYS (uint32; empty where the plan has no such index)"""
    L = plan._lib
    e = handle or L.emu_plan_lower(plan._p)
    if not e:
        raise RuntimeError(L.bc_last_error().decode())
    fields = (C.c_uint32 * len(LAYOUT_FIELDS))()
    ptrs = (C.POINTER(C.c_uint32) * len(LAYOUT_ARRAYS))()
    sizes = (C.c_uint64 * len(LAYOUT_ARRAYS))()
    rc = L.emu_group_layout(e, group, fields, ptrs, sizes)
    out = dict(zip(LAYOUT_FIELDS, (int(v) for v in fields)))
    if rc == 0:
        for name, p, n in zip(LAYOUT_ARRAYS, ptrs, sizes):
            out[name] = np.ctypeslib.as_array(p, shape=(int(n),)).copy() if n else np.zeros(0, dtype=np.uint32)
    if not handle:
        L.emu_plan_destroy(e)
    assert rc == 0
    return out


def emulate(plan, seq, qual, lens, stride, read_len, with_random=False, qlens=None, handle=None):
    """-> (outcomes, dense idx, table entries, discard flag); with_random adds (rcode, rspace): in
    random-barcode mode outcome 0 means "passed every test" -- set membership is the caller's job.
    handle: open_plan(plan), lowered once for many batches (default: lowered here, for this batch)"""
    L = plan._lib  # the emu variant the plan was made with
    e = handle or open_plan(plan)
    n = seq.size // stride
    outc = np.zeros(n, dtype=np.uint8)
    idx = np.zeros(n, dtype=np.uint64)
    rcode = np.zeros(n, dtype=np.uint64)
    rc = L.emu_process2(e, seq.ctypes.data, qual.ctypes.data if qual is not None else None,
                        lens.ctypes.data if lens is not None else None, qlens.ctypes.data if qlens is not None else None,
                        stride, read_len, n, outc.ctypes.data, idx.ctypes.data, rcode.ctypes.data)
    entries = L.emu_table_entries(e)
    discard = L.emu_discard_counts(e)
    rspace = L.emu_rspace(e)
    if not handle:
        L.emu_plan_destroy(e)
    assert rc == 0
    if with_random:
        return outc, idx, entries, discard, rcode, rspace
    return outc, idx, entries, discard
