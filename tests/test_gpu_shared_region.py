"""The specialised match kernel's tile regions (bc_kernel.h, bc_jit.hip: match_shape).  With the quality filter on and the
pipelined fetch, a wave either owns two LDS regions (sequence lines, quality lines: BC_QUAL_REGION=own) or one that
holds, in turn, a tile's sequence lines, its quality lines and the next tile's sequence lines (shared).  Every case runs
both shapes through the C ABI with the specialised kernel forced and compares each of them with the CPU oracle: every
read's outcome, the dense index of every matched read, the six counters and every row.  The batches are the smallest at
which the schedule can go wrong: every wave of the resident grid walks three full tiles and the batch ends in a partial
one; a tile with a byte outside ACGTN and a tile with a quality byte below '!' (both come back to the tile late) sit in
a wave's first, middle and last full tile, with untouched tiles of the same wave before and after."""
import ctypes as C
import os

import numpy as np
import pytest

import parity
import workloads

pytestmark = pytest.mark.gpu

SETS = (4, 20, 20, 20)
R = 100
REGIONS = ["shared", "own"]
COUNTING = ["log", "atomic"]
_cache = {}


@pytest.fixture(autouse=True)
def _forced_kernel(monkeypatch, tmp_path_factory):
    monkeypatch.setenv("BC_JIT", "force")
    monkeypatch.setenv("BC_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit_cache"))


def _env(region, counting):
    env = {"BC_QUAL_REGION": region, "BC_BITMAP_MIN_ENTRIES": "1"}
    if counting == "log":
        env.update(BC_COUNT_LOG="1", BC_COUNT_LOG_MIN_READS="0")
    else:
        env["BC_COUNT_LOG"] = "0"
    return env


def _engine(plan, env):
    """an engine created under `env` (the switches are read at creation), the environment put back afterwards"""
    import ngs_barcode_count_amd as pkg
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pkg.Engine(plan, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _last_launch(eng):
    """(shape key of the specialised kernel, dynamic LDS bytes, grid, workgroups the device holds at once)"""
    key, lds, grid, resident = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    f = eng._lib.bc_internal_last_launch
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    f.restype = C.c_int
    assert f(eng._e, C.byref(key), C.byref(lds), C.byref(grid), C.byref(resident)) == 0
    return key.value, lds.value, grid.value, resident.value


def _workload():
    if "w" not in _cache:
        _cache["w"] = workloads.make("config3", n_sets=SETS, read_len=R)
    return _cache["w"]


def _reads(kind, n, waves):
    """(seq, qual, stride, lens, qlens) of `n` reads, the late readers' bytes planted; shared between the cases"""
    k = (kind, n, waves)
    if k in _cache:
        return _cache[k]
    w = _workload()
    stride = 101 if kind == "stride101" else R
    seq, qual = w.synth.generate_host(0, n, stride)
    seq, qual = seq.reshape(n, stride), qual.reshape(n, stride)
    if stride != R:  # the byte between two reads: plain values
        seq[:, R:] = ord("A")
        qual[:, R:] = ord("I")
    lens = qlens = None
    if kind == "lens":
        rng = np.random.default_rng(7)
        lens = rng.integers(88, R + 1, n).astype(np.uint16)
        qlens = lens.copy()
        cut = rng.random(n) < 0.25  # a quality line shorter than its sequence line
        qlens[cut] -= rng.integers(1, 40, int(cut.sum())).astype(np.uint16)
    # tile t belongs to wave t % waves, as its (t // waves)-th.  (wave, which of its tiles, what): a byte outside ACGTN
    # ('x') or quality bytes below '!' ('q') in a wave's first, middle or last full tile with untouched tiles of the
    # same wave around it; wave 0's last full tile, which the on-demand partial tile follows; every tile of one wave
    plant = [(3, 1, "x"), (5, 1, "q"), (7, 0, "x"), (9, 0, "q"), (11, 2, "x"), (13, 2, "q"), (0, 2, "xq"),
             (15, 0, "xq"), (15, 1, "xq"), (15, 2, "xq")]
    n_full = n // 64
    rows = [(it * waves + wv) * 64 + (wv * 7 + it * 13) % 64 for wv, it, _ in plant if wv < waves and it * waves + wv < n_full]
    what = [k for wv, it, k in plant if wv < waves and it * waves + wv < n_full]
    if n_full <= 1 and n > 9:  # less than a tile, or exactly one
        rows, what = [3, 9], ["x", "q"]
    for r, k in zip(rows, what):
        if "x" in k:
            seq[r, 25] = ord("X")
        if "q" in k:
            qual[r, 10:90:7] = 0x20
    out = (np.ascontiguousarray(seq).reshape(-1), np.ascontiguousarray(qual).reshape(-1), stride, lens, qlens)
    _cache[k] = out
    return out


def _oracle(kind, n, waves):
    """per-read outcomes, counters and rows of the CPU oracle, once per data set"""
    k = ("oracle", kind, n, waves)
    if k not in _cache:
        seq, qual, stride, lens, qlens = _reads(kind, n, waves)
        o = workloads.oracle_for(_workload())
        outc = o.process_batch_outcomes(seq, qual, stride, R, lens=lens, qlens=qlens)
        _cache[k] = (outc, o.counters, o.rows())
    return _cache[k]


def _run(eng, kind, n, waves):
    """submits the data set with tracing on -> (outcomes, dense indices)"""
    import torch
    seq, qual, stride, lens, qlens = _reads(kind, n, waves)
    dseq, dqual = torch.from_numpy(seq).cuda(), torch.from_numpy(qual).cuda()
    outc = torch.zeros(n, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.trace(outc.data_ptr(), idx.data_ptr())
    if lens is not None:
        dl, dq = torch.from_numpy(lens.view(np.int16)).cuda(), torch.from_numpy(qlens.view(np.int16)).cuda()
        torch.cuda.synchronize()
        eng.submit_device_q(dseq.data_ptr(), dqual.data_ptr(), n, stride, dl.data_ptr(), dq.data_ptr())
    else:
        eng.submit_device(dseq.data_ptr(), dqual.data_ptr(), n, stride, R)
    eng.sync()
    eng.trace(None, None)
    return outc.cpu().numpy(), idx.cpu().numpy().astype(np.uint64)


def _check(eng, kind, n, waves, counting, folds_before=0):
    outc, idx = _run(eng, kind, n, waves)
    exp_outc, exp_counters, exp_rows = _oracle(kind, n, waves)
    bad = np.nonzero(outc != exp_outc)[0]
    assert bad.size == 0, (bad[:8], outc[bad[:8]], exp_outc[bad[:8]], "tiles", np.unique(bad // 64)[:8])
    matched = exp_outc == parity.CODE["matched"]
    di, cnt = np.unique(idx[matched], return_counts=True)
    plan = _workload().plan
    assert parity.decode_rows(plan, dict(zip(di.tolist(), cnt.tolist())), False) == exp_rows
    assert eng.kernel_name().startswith("bc_jit_match_count"), eng.kernel_name()
    folds = eng.count_log_folds() - folds_before
    assert (folds > 0) if counting == "log" else (folds == 0), folds
    return exp_counters, exp_rows


def _resident_waves(eng, kind):
    """the waves of a full grid of this engine's launches of this shape, from a launch of one tile"""
    _run(eng, kind, 64, 1)
    _, _, _, resident = _last_launch(eng)
    assert resident >= 1
    eng.reset()
    return resident * 4, eng.count_log_folds()


@pytest.mark.parametrize("counting", COUNTING)
@pytest.mark.parametrize("region", REGIONS)
@pytest.mark.parametrize("kind", ["fixed", "stride101", "lens"])
def test_three_tiles_per_wave_and_a_partial_one(kind, region, counting):
    eng = _engine(_workload().plan, _env(region, counting))
    waves, folds0 = _resident_waves(eng, kind)
    n = 3 * waves * 64 + 37
    counters, rows = _check(eng, kind, n, waves, counting, folds0)
    _, _, grid, resident = _last_launch(eng)
    assert grid == resident  # the whole resident grid ran, every wave three full tiles
    got = eng.counters()
    assert {k: got[k] for k in counters} == counters
    assert got["total_reads"] == n and got["unsupported_reads"] == 0
    assert eng.result_rows() == rows
    eng.close()


@pytest.mark.parametrize("counting", COUNTING)
@pytest.mark.parametrize("region", REGIONS)
@pytest.mark.parametrize("n", [37, 64])
def test_less_than_a_tile_and_exactly_one(n, region, counting):
    eng = _engine(_workload().plan, _env(region, counting))
    counters, rows = _check(eng, "fixed", n, 1, counting)
    got = eng.counters()
    assert {k: got[k] for k in counters} == counters
    assert eng.result_rows() == rows
    eng.close()


def _match_shape(plan, stride, read_len, qshare):
    """match_shape of a plan on an MI355X (no device involved): (key, LDS with the hot-counter cache, LDS without it,
    region bytes, exact-match table bytes, shared shape chosen)"""
    f = plan._lib.bc_internal_match_shape
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64)] + [C.POINTER(C.c_uint32)] * 4 + \
                 [C.POINTER(C.c_int)]
    f.restype = C.c_int
    key, shared = C.c_uint64(), C.c_int()
    v = [C.c_uint32() for _ in range(4)]
    assert f(plan._p, stride, read_len, 0, 1 if qshare else 0, C.byref(key), *[C.byref(x) for x in v], C.byref(shared)) == 0
    return (key.value,) + tuple(x.value for x in v) + (bool(shared.value),)


HOT_BYTES = 256 * 8  # bc_kernel.h: kHotBytes
REGION = (64 * R + 4 * 32 + 16 + 15) & ~15  # match_shape: 64 reads + the slack behind them


def test_shape_key_and_lds():
    """the two shapes are two kernels (engine key, hence code-object cache entry); the shared one asks for four regions
    less; both are what the launch really asks for, with and without the hot-counter cache.  A plan without the quality
    filter has one region either way: the same key and the LDS it always had, four regions and the tables (and the
    cache where it is on)"""
    import torch
    w = _workload()
    seen = {}
    for region in REGIONS:
        key, hot, cold, reg, tables, shared = _match_shape(w.plan, R, R, region == "shared")
        assert reg == REGION and shared == (region == "shared")
        assert cold == (4 if shared else 8) * REGION + tables and hot == cold + HOT_BYTES
        for counting in COUNTING:
            eng = _engine(w.plan, _env(region, counting))
            _run(eng, "fixed", 64, 1)
            assert _last_launch(eng)[:2] == (key, cold if counting == "log" else hot)
            eng.close()
        seen[region] = key
    assert seen["shared"] != seen["own"]
    plain = workloads.make("config2", n_sets=SETS, read_len=R)
    seq, _ = plain.synth.generate_host(0, 64)
    shapes = [_match_shape(plain.plan, R, R, q) for q in (True, False)]
    assert shapes[0] == shapes[1] and not shapes[0][5]
    key, hot, cold, reg, tables, _ = shapes[0]
    assert cold == 4 * REGION + tables and hot == cold + HOT_BYTES
    for region in REGIONS:
        for counting in COUNTING:
            eng = _engine(plain.plan, _env(region, counting))
            dseq = torch.from_numpy(seq).cuda()
            torch.cuda.synchronize()
            eng.submit_device(dseq.data_ptr(), None, 64, R, R)
            eng.sync()
            assert eng.kernel_name().startswith("bc_jit_match_count")
            # (an engine without tracing: the key's trace bit is the only difference)
            assert _last_launch(eng)[1] == (cold if counting == "log" else hot)
            assert _last_launch(eng)[0] | 1 == key | 1
            eng.close()
