"""The tile loop of the specialised match kernel in every counting variant the engine can choose beneath one shape key
(bc_jit.h JitVariant: through the log with the hot-counter cache off or on, bit map + atomics, plain atomics), at the
read counts where 32-bit tile numbers, the partial last tile and the packed outcome counters can go wrong: less than a
tile, exactly one, one read more, one read more than a tile per resident wave, fewer tiles than waves, and two tiles per
wave plus a partial one.  Config-3-shaped plan with small sets, 100-base reads, quality filter on; every read's outcome
and dense index, the counters and the rows against the CPU oracle.  Every batch carries a byte outside ACGTN ("x") or
quality bytes below '!' ("q") in the first read of a full tile and in the last read of the partial one.
BC_PIPE=0 (fetch on demand: every tile goes through the staged body) is honoured by -DBC_EXPERIMENT builds only; the
release library never launches a specialised kernel unpipelined (only strides of 315-320 bases are, and they run the
generic kernel), so that case skips unless BC_LIB names an experiment build.  The packed counters' field arithmetic:
tests/test_outcome_pack.py (no GPU needed); no test here gives a wave the 255 tiles after which the kernel sums them
mid-launch -- that takes 64 x 255 reads per resident wave, 67 M reads on an MI355X, and there is no hook to shrink the
grid -- so that flush runs in launches of the benchmark's size only (100 M reads: 381 tiles per wave), where
bench.py and tools/ab_bench.py compare the counters with the CPU's and the parent build's."""
import ctypes as C
import os

import numpy as np
import pytest

import parity
import workloads

pytestmark = pytest.mark.gpu

SETS = (4, 40, 40, 40)
R = 100
# environment of an engine per counting variant (read when the engine is created)
VARIANTS = {
    "log": dict(BC_BITMAP_MIN_ENTRIES="1", BC_COUNT_LOG="1", BC_COUNT_LOG_MIN_READS="0", BC_COUNT_LOG_HOT="0"),
    "log_hot": dict(BC_BITMAP_MIN_ENTRIES="1", BC_COUNT_LOG="1", BC_COUNT_LOG_MIN_READS="0", BC_COUNT_LOG_HOT="1"),
    "bitmap": dict(BC_BITMAP_MIN_ENTRIES="1", BC_COUNT_LOG="0"),
    "atomic": dict(BC_BITMAP_MIN_ENTRIES=str(1 << 40), BC_COUNT_LOG="0"),
}
SIZES = ["1", "63", "64", "65", "waves+1", "half", "two+partial"]
_cache = {}


@pytest.fixture(autouse=True)
def _forced_kernel(monkeypatch, tmp_path_factory):
    monkeypatch.setenv("BC_JIT", "force")
    monkeypatch.setenv("BC_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit_cache_tile_loop"))


def _workload():
    if "w" not in _cache:
        _cache["w"] = workloads.make("config3", n_sets=SETS, read_len=R)
    return _cache["w"]


def _engine(env):
    import ngs_barcode_count_amd as pkg
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pkg.Engine(_workload().plan, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _last_launch(eng):
    key, lds, grid, resident = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    f = eng._lib.bc_internal_last_launch
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    f.restype = C.c_int
    assert f(eng._e, C.byref(key), C.byref(lds), C.byref(grid), C.byref(resident)) == 0
    return key.value, lds.value, grid.value, resident.value


def _n_reads(size, waves):
    return {"waves+1": 64 * waves + 1, "half": 64 * (waves // 2) + 5, "two+partial": 2 * 64 * waves + 37}.get(size) or int(size)


def _reads(n, plant):
    k = ("reads", n, plant)
    if k not in _cache:
        seq, qual = _workload().synth.generate_host(0, n)
        seq, qual = seq.reshape(n, R).copy(), qual.reshape(n, R).copy()
        rows = ([0] if n >= 64 else []) + ([n - 1] if n % 64 else [])  # first read of a full tile, last of the partial one
        for r in rows:
            if plant == "x":
                seq[r, 25] = ord("X")
            else:
                qual[r, 10:90:7] = 0x20
        _cache[k] = (seq.reshape(-1), qual.reshape(-1))
    return _cache[k]


def _oracle(n, plant):
    k = ("oracle", n, plant)
    if k not in _cache:
        seq, qual = _reads(n, plant)
        o = workloads.oracle_for(_workload())
        outc = o.process_batch_outcomes(seq, qual, R, R)
        _cache[k] = (outc, o.counters, o.rows())
    return _cache[k]


def _run(eng, n, plant, trace=True):
    import torch
    seq, qual = _reads(n, plant)
    dseq, dqual = torch.from_numpy(seq).cuda(), torch.from_numpy(qual).cuda()
    outc = torch.zeros(n, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    if trace:
        eng.trace(outc.data_ptr(), idx.data_ptr())
    eng.submit_device(dseq.data_ptr(), dqual.data_ptr(), n, R, R)
    eng.sync()
    if trace:
        eng.trace(None, None)
    return outc.cpu().numpy(), idx.cpu().numpy().astype(np.uint64)


def _resident_waves(eng):
    """waves of a full grid of this engine's launches, from a launch of one tile (the engine is reset afterwards)"""
    _run(eng, 64, "x")
    resident = _last_launch(eng)[3]
    assert resident >= 1
    eng.reset()
    return resident * 4


def _check(eng, n, plant, variant, trace=True):
    folds0 = eng.count_log_folds()
    outc, idx = _run(eng, n, plant, trace)
    exp_outc, exp_counters, exp_rows = _oracle(n, plant)
    assert eng.kernel_name().startswith("bc_jit_match_count"), eng.kernel_name()
    folds = eng.count_log_folds() - folds0
    assert (folds > 0) if variant.startswith("log") else (folds == 0), folds
    if trace:
        bad = np.nonzero(outc != exp_outc)[0]
        assert bad.size == 0, (bad[:8], outc[bad[:8]], exp_outc[bad[:8]], "tiles", np.unique(bad // 64)[:8])
        matched = exp_outc == parity.CODE["matched"]
        di, cnt = np.unique(idx[matched], return_counts=True)
        assert parity.decode_rows(_workload().plan, dict(zip(di.tolist(), cnt.tolist())), False) == exp_rows
    got = eng.counters()
    assert {k: got[k] for k in exp_counters} == exp_counters
    assert got["total_reads"] == n and got["unsupported_reads"] == 0
    assert eng.result_rows() == exp_rows


@pytest.mark.parametrize("plant", ["x", "q"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_sizes_in_every_counting_variant(variant, size, plant):
    eng = _engine(VARIANTS[variant])
    waves = _resident_waves(eng)
    n = _n_reads(size, waves)
    _check(eng, n, plant, variant)
    eng.close()


@pytest.mark.parametrize("size", ["65", "two+partial"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_without_trace(variant, size):
    """the kernel an untraced engine runs (the shape key's trace bit apart): counters and rows"""
    eng = _engine(VARIANTS[variant])
    waves = _resident_waves(eng)
    _check(eng, _n_reads(size, waves), "x", variant, trace=False)
    eng.close()


@pytest.mark.parametrize("size", ["63", "65", "two+partial"])
@pytest.mark.parametrize("variant", ["log", "bitmap"])
def test_fetch_on_demand(variant, size):
    eng = _engine(dict(VARIANTS[variant], BC_PIPE="0"))
    waves = _resident_waves(eng)
    # an unpipelined launch never shares its region (match_shape): bit 15 of the key says whether BC_PIPE was honoured
    if _last_launch(eng)[0] & (1 << 15):
        eng.close()
        pytest.skip("this library ignores BC_PIPE (not an experiment build): it has no unpipelined specialised launch")
    _check(eng, _n_reads(size, waves), "q", variant)
    eng.close()


def test_variants_share_the_shape_key(tmp_path, monkeypatch):
    """the counting variant is beneath the key: every variant of one shape reports the same key, after a precompile
    that builds the variants the engine chooses between"""
    import ngs_barcode_count_amd as pkg
    w = _workload()
    monkeypatch.setenv("BC_JIT_CACHE", str(tmp_path / "fresh_cache"))  # only what the precompile builds is in it
    old = os.environ.get("BC_BITMAP_MIN_ENTRIES")
    os.environ["BC_BITMAP_MIN_ENTRIES"] = "1"
    try:
        pkg.precompile(w.plan, stride=R, read_len=R, cache_dir=os.environ["BC_JIT_CACHE"])
    finally:
        if old is None:
            del os.environ["BC_BITMAP_MIN_ENTRIES"]
        else:
            os.environ["BC_BITMAP_MIN_ENTRIES"] = old
    keys = {}
    for variant in ("log", "bitmap"):
        eng = _engine(dict(VARIANTS[variant], BC_JIT="cached"))  # cache hits only: nothing is compiled at the launch
        _run(eng, 64, "x", trace=False)
        assert eng.kernel_name().startswith("bc_jit_match_count"), (variant, eng.kernel_name())
        keys[variant] = _last_launch(eng)[0]
        eng.close()
    assert keys["log"] == keys["bitmap"] and keys["log"] != 0
