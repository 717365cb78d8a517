"""The seams between the match kernels.  A batch reaches the lane-per-read kernel (eight <NW,NWW> instantiations), its
scheme-specialised form or the wave-per-read kernel (bc_long.h) by the longest read it can hold and the scheme's length
alone, so the kernel can change from one submit to the next on ONE engine -- a FASTQ file whose first record above 320
bases comes part way through does just that -- while table, bit map, hash set or map stay the same.  Here: both sides of
every dispatch edge by kernel name; jobs that mix the kernels on one engine in every counting mode, read back through
finish, nonzero_entries, enrichment and the text renderers; resets across the seam; such a FASTQ file; and the
wave-per-read kernel's quality edges.  Everything is compared with the CPU oracle: every read's outcome and index
(parity.check_per_read; with a random barcode matched/duplicate are one class), the six counters and every row."""
import os

import numpy as np
import pytest

import cases
import parity
import seam_cases as sc
from test_gpu_enrich import assert_same, marginals, sizes_of
from test_gpu_parity import make_plan
from test_gpu_render import expected_counts, expected_merged, ids_of, n_samples_of

pytestmark = pytest.mark.gpu

LONG = "long_match_kernel"
BITS = {"BC_BITMAP_MIN_ENTRIES": "1"}
MODES = {"default": {}, "bitmap_atomic": dict(BITS, BC_COUNT_LOG="0"), "bitmap_log": dict(BITS, BC_COUNT_LOG="1")}
_cache = {}


def _pkg():
    import ngs_barcode_count_amd as pkg
    return pkg


def _engine(plan, env=None, **kw):
    """an engine created under `env` (the switches are read at creation), the environment put back afterwards"""
    old = {k: os.environ.get(k) for k in env or {}}
    os.environ.update(env or {})
    try:
        return _pkg().Engine(plan, device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture
def generic(monkeypatch):
    monkeypatch.setenv("BC_JIT", "0")


@pytest.fixture
def specialised(monkeypatch, tmp_path_factory):
    monkeypatch.setenv("BC_JIT", "force")
    monkeypatch.setenv("BC_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit_cache"))


def _plan(c):
    k = ("plan", c["name"])
    if k not in _cache:
        _cache[k] = make_plan(c)
    return _cache[k]


def _submit(eng, b, lens=None, qlens=None):
    """one batch (seam_cases.make_batch) into `eng`, traced, not synced -> the buffers (kept alive by the caller)"""
    import torch
    n = b["seq"].size // b["stride"]
    lens = b["lens"] if lens is None else lens
    h = dict(n=n, seq=torch.from_numpy(b["seq"]).cuda(), qual=torch.from_numpy(b["qual"]).cuda(),
             lens=torch.from_numpy(lens.view(np.int16)).cuda() if lens is not None else None,
             qlens=torch.from_numpy(qlens.view(np.int16)).cuda() if qlens is not None else None,
             outc=torch.full((n,), 255, dtype=torch.uint8, device="cuda"), idx=torch.zeros(n, dtype=torch.int64, device="cuda"))
    assert h["seq"].data_ptr() % 16 == 0 and h["qual"].data_ptr() % 16 == 0
    torch.cuda.synchronize()
    eng.trace(h["outc"].data_ptr(), h["idx"].data_ptr())
    if qlens is not None:
        eng.submit_device_q(h["seq"].data_ptr(), h["qual"].data_ptr(), n, b["stride"], h["lens"].data_ptr(), h["qlens"].data_ptr())
    else:
        eng.submit_device(h["seq"].data_ptr(), h["qual"].data_ptr(), n, b["stride"], b["read_len"],
                          h["lens"].data_ptr() if h["lens"] is not None else None)
    eng.trace(None, None)
    return h


def _traced(h):
    return h["outc"].cpu().numpy(), h["idx"].cpu().numpy().astype(np.uint64)


def _check_reads(c, plan, h, reads):
    """every read's outcome and index against the oracle; -> that batch's oracle"""
    outc, idx = _traced(h)
    one = dict(c, reads=reads)
    if not plan.random_barcode:
        return parity.check_per_read(one, plan, outc, idx, False)
    # which copy of a PCR duplicate is the matched one depends on scheduling: matched / duplicate are one class
    o = parity.oracle_for(one)
    fold = lambda v: 0 if v == parity.CODE["duplicates"] else v
    for i, (s, q) in enumerate(reads):
        e = o.process(s, q)
        assert fold(int(outc[i])) == fold(parity.CODE[e]), (i, e, int(outc[i]))
    return o


def _oracle_over(c, batches):
    """counters and rows of the oracle over the batches in order (one Results)"""
    k = ("over", c["name"], tuple(batches))
    if k not in _cache:
        o = parity.oracle_for(c)
        for name in batches:
            b = c["batches"][name]
            o.process_batch(b["seq"], b["qual"], b["stride"], b["read_len"], lens=b["lens"])
        _cache[k] = (o.counters, o.rows())
    return _cache[k]


def _check_totals(eng, counters, rows, n_reads):
    got = eng.counters()
    assert {k: got[k] for k in counters} == counters, (got, counters)
    assert got["total_reads"] == n_reads and got["unsupported_reads"] == 0
    assert eng.result_rows() == rows


def _one_shape(c, b, name):
    """one batch on a fresh engine: per-read parity, counters, rows and the kernel that ran"""
    plan = _plan(c)
    eng = _engine(plan)
    h = _submit(eng, b)
    got = eng.kernel_name()
    eng.sync()
    o = _check_reads(c, plan, h, b["reads"])
    _check_totals(eng, o.counters, o.rows(), h["n"])
    assert o.counters["matched"] > 0
    eng.close()
    if callable(name):
        assert name(got), got
    else:
        assert got == name, (got, name)


# ---------------------------------------------------------------------------------------------------------------------
# 1. every instantiation, both sides of every edge
# ---------------------------------------------------------------------------------------------------------------------
_EDGES = [("nosample", m, t) for m, t in sc.NOSAMPLE_EDGES] + [("long_l", m, t) for m, t in sc.LONG_L_EDGES]


def test_the_edge_lists_name_every_kernel():
    tags = {t for _, _, t in _EDGES}
    assert tags == {"<4,1>", "<4,2>", "<4,4>", "<8,2>", "<8,4>", "<8,8>", "<10,4>", "<10,10>", "long"}
    for which, m, t in _EDGES:  # the table of the dispatch, restated in seam_cases.lane_kernel
        assert sc.lane_kernel(m, sc.SWEEP_L[which]) == sc.expected_kernel(t), (which, m)


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
@pytest.mark.parametrize("which,maxlen,tag", _EDGES, ids=["%s-%d" % (w, m) for w, m, _ in _EDGES])
def test_generic_kernel_at_every_dispatch_edge(generic, which, maxlen, tag, ragged):
    c = sc.SWEEP_CASES[which]()
    b = sc.shape_batch(which, maxlen, ragged)
    assert b["stride"] == maxlen and (b["lens"] is not None) == ragged
    _one_shape(c, b, sc.expected_kernel(tag))


@pytest.mark.parametrize("which,maxlen,jit", sc.JIT_SHAPES, ids=["%s-%d" % (w, m) for w, m, _ in sc.JIT_SHAPES])
def test_specialised_kernel_up_to_its_last_shape(specialised, which, maxlen, jit):
    """<8,4> is the last instantiation the specialised kernel serves: NOSAMPLE at 161 and LONG_L at 256 bases run it,
    one base more stays on the generic kernel (fixed and ragged shapes in turn)"""
    c = sc.SWEEP_CASES[which]()
    b = sc.shape_batch(which, maxlen, ragged=bool(maxlen % 2))
    generic_name = sc.lane_kernel(maxlen, sc.SWEEP_L[which])
    _one_shape(c, b, (lambda got: got.startswith("bc_jit_match_count<")) if jit else generic_name)


def _last_lds(eng):
    """dynamic LDS bytes of the engine's last match launch"""
    import ctypes as C
    key, lds, grid, resident = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    f = eng._lib.bc_internal_last_launch
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    f.restype = C.c_int
    assert f(eng._e, C.byref(key), C.byref(lds), C.byref(grid), C.byref(resident)) == 0
    return lds.value


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
def test_two_tile_regions_stop_fitting_at_315_bases(generic, ragged):
    """with the quality filter on, the pipelined fetch keeps a sequence and a quality region per wave: 8 regions of
    64 x stride bytes (+ 336 of slack) fit the 160 KiB of LDS up to 314 bases.  From 315 on the batch is fetched on
    demand into one region per wave (every tile then goes the way of a partial one) -- it used to be refused with
    "read stride too large for one LDS tile", as test_generic_kernel_at_every_dispatch_edge[*-320-*] showed"""
    c = sc.nosample_case()
    plan = _plan(c)
    lds = {}
    for maxlen in (314, 315):
        b = sc.shape_batch("nosample", maxlen, ragged)
        eng = _engine(plan)
        h = _submit(eng, b)
        assert eng.kernel_name() == "match_count_kernel<10,10>"
        lds[maxlen] = _last_lds(eng)
        eng.sync()
        o = _check_reads(c, plan, h, b["reads"])
        _check_totals(eng, o.counters, o.rows(), h["n"])
        assert o.counters["matched"] > 0 and o.counters["low_quality"] > 0
        eng.close()
    region = lambda stride: (64 * stride + 10 * 32 + 16 + 15) & ~15
    assert lds == {314: 8 * region(314), 315: 4 * region(315)}


def test_same_reads_through_every_stride(generic):
    """one pool of ragged reads, submitted with lengths at strides either side of 256 and 320: <8,8>, <10,10> and the
    wave-per-read kernel give the same outcome and index for every read"""
    c = sc.same_reads_pool()
    plan = _plan(c)
    seen, first = [], None
    for stride, tag in sc.POOL_STRIDES:
        b = sc.make_batch(c["reads"], stride=stride, use_lens=True)
        eng = _engine(plan)
        h = _submit(eng, b)
        seen.append(eng.kernel_name())
        assert seen[-1] == sc.expected_kernel(tag), (stride, seen[-1])
        eng.sync()
        outc, idx = _traced(h)
        if first is None:
            o = parity.check_per_read(c, plan, outc, idx, False)
            first = (outc, idx, o.counters, o.rows())
            assert o.counters["matched"] > 100 and o.counters["low_quality"] > 0
        matched = first[0] == 0
        assert np.array_equal(outc, first[0]), stride
        assert np.array_equal(idx[matched], first[1][matched]), stride
        _check_totals(eng, first[2], first[3], len(c["reads"]))
        eng.close()
    assert len(set(seen)) == 3


# ---------------------------------------------------------------------------------------------------------------------
# 2. mixed jobs on one engine
# ---------------------------------------------------------------------------------------------------------------------
def _expected_name(plan, b):
    return sc.lane_kernel(b["stride"] if b["use_lens"] else b["read_len"], plan.length)


def _run_order(c, eng, order):
    """the batches of `order` into `eng`, no sync between them; the kernel asserted after every submit -> handles"""
    plan = eng.plan
    hs, names = [], []
    for name in order:
        b = c["batches"][name]
        hs.append(_submit(eng, b))
        names.append(eng.kernel_name())
        assert names[-1] == _expected_name(plan, b), (name, names[-1])
        assert (names[-1] == LONG) == (name in sc.LONG_BATCHES)
    assert LONG in names and any(n.startswith("match_count_kernel<") for n in names)  # both families on this engine
    return hs


def _index_maps(plan, rows):
    """oracle rows -> {sample index: {tuple index: count}}, the sizes of the counted sets, and Engine.rows()' arrays"""
    samples = {x: i for i, (x, _) in enumerate(plan.samples())} if plan.sample_barcode else {"barcode": 0}
    sets = [{x: i for i, (x, _) in enumerate(plan.counted(g))} for g in range(plan.barcode_num)]
    sizes = [len(s) for s in sets]
    maps = {i: {} for i in range(n_samples_of(plan))}
    s_idx, b_idx, cnt = [], [], []
    for sample, tup, n in rows:
        digits = [sets[g][x] for g, x in enumerate(tup.split(","))]
        t = 0
        for g, d in enumerate(digits):
            t = t * sizes[g] + d
        maps[samples[sample]][t] = n
        s_idx.append(samples[sample])
        b_idx.append(digits)
        cnt.append(n)
    return maps, sizes, (np.array(s_idx), np.array(b_idx).reshape(len(rows), len(sizes)), np.array(cnt, dtype=np.uint64))


def _check_readers_unsynced(eng, rows):
    """nonzero_entries, enrichment and the renderers read bits and table as they stand, straight after a submit"""
    plan = eng.plan
    maps, sizes, (s, b, cnt) = _index_maps(plan, rows)
    assert eng.nonzero_entries() == len(rows)
    assert_same(eng.enrichment(), marginals(s, b, cnt, n_samples_of(plan), sizes_of(plan)))
    ids = ids_of(plan)
    S = n_samples_of(plan)
    for sample in range(S):
        assert eng.render_counts(sample) == expected_counts(maps, sizes, ids, sample), sample
    assert eng.render_merged(list(range(S))) == expected_merged(maps, sizes, ids, list(range(S)))


def test_small_batches_share_their_rows():
    """the mixing means something only if lane and wave-per-read batches add to the SAME table entries: at least half
    of all rows get counts from P4 and also from a lane batch"""
    c = sc.small("plain")
    per = {}
    for name in ("P1", "P2", "P3", "P4"):
        _, rows = _oracle_over(c, (name,))
        per[name] = {(s, t) for s, t, _ in rows}
    every = set().union(*per.values())
    both = per["P4"] & (per["P1"] | per["P2"] | per["P3"])
    print("rows", len(every), "from P4 and a lane batch", len(both))
    assert 2 * len(both) >= len(every) and len(every) <= 375


@pytest.mark.parametrize("order", sc.ORDERS, ids=["-".join(o) for o in sc.ORDERS])
@pytest.mark.parametrize("mode", list(MODES))
def test_mixed_job_dense(generic, mode, order):
    c = sc.small("plain")
    plan = _plan(c)
    assert plan.mode == "dense" and plan.table_entries == 375
    eng = _engine(plan, MODES[mode])
    hs = _run_order(c, eng, order)
    counters, rows = _oracle_over(c, order)
    if mode != "default":
        _check_readers_unsynced(eng, rows)
    eng.sync()
    for h, name in zip(hs, order):
        _check_reads(c, plan, h, c["batches"][name]["reads"])
    _check_totals(eng, counters, rows, 1200 * len(order))
    lane_submits = sum(1 for name in order if name not in sc.LONG_BATCHES)
    assert eng.count_log_folds() == (lane_submits if mode == "bitmap_log" else 0)
    if mode != "default":
        _check_readers_unsynced(eng, rows)  # and once more after finish() has run
    eng.close()


@pytest.mark.parametrize("order", sc.ORDERS, ids=["-".join(o) for o in sc.ORDERS])
def test_mixed_job_random_barcode(generic, order):
    """one hash set of (tuple, random barcode) keys under both kernels: in [P1, P5] every read of P5 is a duplicate of
    one that the lane kernel inserted"""
    c = sc.small("random")
    plan = _plan(c)
    assert plan.random_barcode and plan.mode == "dense"
    eng = _engine(plan)
    hs = _run_order(c, eng, order)
    eng.sync()
    for h, name in zip(hs, order):
        _check_reads(c, plan, h, c["batches"][name]["reads"])
    counters, rows = _oracle_over(c, order)
    _check_totals(eng, counters, rows, 1200 * len(order))
    assert eng.key_count() == counters["matched"] and counters["duplicates"] > 0
    if order == ("P1", "P5"):
        alone, _ = _oracle_over(c, ("P1",))
        assert counters["matched"] == alone["matched"]
        assert counters["duplicates"] == 2 * alone["duplicates"] + alone["matched"]
    eng.close()


@pytest.mark.parametrize("order", sc.ORDERS, ids=["-".join(o) for o in sc.ORDERS])
def test_mixed_job_raw_keys(generic, order):
    """narrow raw keys: one map of (key, count) under both kernels"""
    c = sc.small("raw")
    plan = _plan(c)
    assert plan.mode == "sparse" and not plan.random_barcode
    eng = _engine(plan)
    hs = _run_order(c, eng, order)
    eng.sync()
    for h, name in zip(hs, order):
        _check_reads(c, plan, h, c["batches"][name]["reads"])
    counters, rows = _oracle_over(c, order)
    _check_totals(eng, counters, rows, 1200 * len(order))
    assert counters["matched"] > 0 and max(n for _, _, n in rows) > 1
    eng.close()


def test_mixed_job_on_a_caller_owned_table(generic):
    import torch
    c = sc.small("plain")
    plan = _plan(c)
    tables = [torch.zeros(plan.table_entries, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    eng = _engine(plan, MODES["bitmap_log"], table_ptr=tables[0].data_ptr())
    ref = _engine(plan, {"BC_COUNT_LOG": "0", "BC_BITMAP_MIN_ENTRIES": str(1 << 26)}, table_ptr=tables[1].data_ptr())
    order = ("P1", "P4")
    keep = []
    for e in (eng, ref):
        keep.append(_run_order(c, e, order))
        e.sync()
    counters, rows = _oracle_over(c, order)
    assert torch.equal(tables[0], tables[1])
    assert int(tables[0].sum()) == counters["matched"]
    assert (eng.count_log_folds(), ref.count_log_folds()) == (1, 0)
    for e in (eng, ref):
        _check_totals(e, counters, rows, 2400)
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. resets across the seam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switches", [{}, {"BC_COUNT_LOG_DEFER_RESET": "0", "BC_COUNT_LOG_FRESH": "0"}], ids=["default", "neither"])
def test_resets_across_the_seam(generic, switches):
    """four jobs on one engine, bit map and log forced: a whole-table reset owed after a wave-per-read launch (job 2),
    that kernel meeting an owed reset (job 3), a fresh fold following it (job 4)"""
    c = sc.small("plain")
    plan = _plan(c)
    env = dict(MODES["bitmap_log"], **switches)
    eng = _engine(plan, env)
    jobs = [(("P1", "P4"), "reset_results"), (("P2",), "reset"), (("P4",), "reset"), (("P1",), None)]
    carried = dict.fromkeys(parity.CODE, 0)  # what reset_results lets run on
    reads_carried = 0
    folds = 0
    for order, after in jobs:
        hs = []
        for name in order:
            hs.append(_submit(eng, c["batches"][name]))
            assert eng.kernel_name() == _expected_name(plan, c["batches"][name])
        counters, rows = _oracle_over(c, order)
        got_rows = eng.result_rows()
        assert got_rows == rows, order
        fresh = _engine(plan, dict(BITS, BC_COUNT_LOG="0"))
        keep = [_submit(fresh, c["batches"][name]) for name in order]
        assert got_rows == fresh.result_rows(), order
        assert fresh.count_log_folds() == 0
        fresh.close()
        del keep
        got = eng.counters()
        assert {k: got[k] for k in counters} == {k: counters[k] + carried[k] for k in counters}, order
        assert got["total_reads"] == reads_carried + 1200 * len(order)
        folds += sum(1 for name in order if name not in sc.LONG_BATCHES)
        assert eng.count_log_folds() == folds
        _check_readers_unsynced(eng, rows)
        if after == "reset_results":
            eng.reset_results()
            carried = {k: counters[k] + carried[k] for k in counters}
            reads_carried += 1200 * len(order)
        elif after == "reset":
            eng.reset()
            carried = dict.fromkeys(parity.CODE, 0)
            reads_carried = 0
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. a FASTQ file that crosses 320 bases part way through
# ---------------------------------------------------------------------------------------------------------------------
def _fastq_parts():
    if "fastq" not in _cache:
        c = sc.small("plain")
        head = sc.fastq_records(c, [(1500, 56, 150)], seed=4401)
        long_ = sc.fastq_records(c, [(40, 330, 400)], seed=4402)
        tail = sc.fastq_records(c, [(500, 56, 150)], seed=4403)
        _cache["fastq"] = (head, long_, tail)
    return _cache["fastq"]


def _oracle_reads(c, reads):
    o = parity.oracle_for(c)
    for s, q in reads:
        o.process(s, q)
    return o.counters, o.rows()


@pytest.mark.parametrize("mode", ["default", "bitmap_log"])
def test_fastq_crossing_320_bases_mid_file(generic, mode, tmp_path, monkeypatch):
    monkeypatch.setenv("BC_INGEST_CHUNK", "4096")
    c = sc.small("plain")
    head, long_, tail = _fastq_parts()
    reads = head + long_ + tail
    path = tmp_path / "crossing.fastq"
    path.write_bytes(sc.fastq_text(reads))
    eng = _engine(_plan(c), MODES[mode])
    assert eng.count_fastq(path) == len(reads)
    assert eng.kernel_name() == LONG  # (ragged chunks keep the widest stride seen: the tail runs on this kernel too)
    counters, rows = _oracle_reads(c, reads)
    _check_totals(eng, counters, rows, len(reads))
    assert counters["matched"] > 500
    if mode == "bitmap_log":
        assert eng.count_log_folds() > 0  # the chunks ahead of the first long record
    eng.close()


@pytest.mark.parametrize("mode", ["default", "bitmap_log"])
def test_two_fastq_files_into_one_engine(generic, mode, tmp_path, monkeypatch):
    monkeypatch.setenv("BC_INGEST_CHUNK", "4096")
    c = sc.small("plain")
    head, long_, tail = _fastq_parts()
    first, second = tmp_path / "short.fastq", tmp_path / "long.fastq"
    first.write_bytes(sc.fastq_text(head))
    second.write_bytes(sc.fastq_text(tail[:100] + long_ + tail[100:], first=len(head)))
    eng = _engine(_plan(c), MODES[mode])
    assert eng.count_fastq(first) == len(head)
    assert eng.kernel_name().startswith("match_count_kernel<")
    folds = eng.count_log_folds()
    assert (folds > 0) == (mode == "bitmap_log")
    assert eng.count_fastq(second) == len(long_) + len(tail)
    assert eng.kernel_name() == LONG
    reads = head + tail[:100] + long_ + tail[100:]
    counters, rows = _oracle_reads(c, reads)
    _check_totals(eng, counters, rows, len(reads))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. quality edges of the wave-per-read kernel
# ---------------------------------------------------------------------------------------------------------------------
def _short_quality_lines(c, b):
    """qlens for P4 at stride 336: shorter than the sequence line for half the reads.  A random cut changes next to no
    outcome, so reads whose uncut outcome is low_quality get theirs inside the matched construct, just ahead of the
    first low score (the run that failed them is cut off); the others get a cut anywhere, some of them 0, some a few
    bases into the read (ahead of where most matches start)"""
    rng = np.random.default_rng(4501)
    n = len(b["reads"])
    o = parity.oracle_for(c)
    uncut = o.process_batch_outcomes(b["seq"], b["qual"], b["stride"], b["stride"], lens=b["lens"])
    qlens = b["lens"].copy()
    low = np.flatnonzero(uncut == parity.CODE["low_quality"])
    for i in low:
        q = b["reads"][i][1]
        p = next(k for k, ch in enumerate(q) if ord(ch) - 33 < 16)
        qlens[i] = max(p - int(rng.integers(0, 3)), 0)
    rest = np.setdiff1d(np.arange(n), low)
    pick = rng.choice(rest, n // 2 - low.size, replace=False)
    for j, i in enumerate(pick):
        full = int(b["lens"][i])
        qlens[i] = 0 if j % 10 == 0 else (int(rng.integers(1, 12)) if j % 10 == 1 else int(rng.integers(0, full)))
    return uncut, qlens


def test_wave_per_read_kernel_short_quality_lines(generic):
    c = sc.small("plain")
    plan = _plan(c)
    b = sc.make_batch(c["batches"]["P4"]["reads"], stride=336, use_lens=True)
    uncut, qlens = _short_quality_lines(c, b)
    n = len(b["reads"])
    assert int((qlens < b["lens"]).sum()) == n // 2 and int((qlens == 0).sum()) > 0
    o = parity.oracle_for(c)
    exp = o.process_batch_outcomes(b["seq"], b["qual"], b["stride"], b["stride"], lens=b["lens"], qlens=qlens)
    changed = int((exp != uncut).sum())
    print("outcomes the cut changes:", changed)
    assert changed >= 20
    eng = _engine(plan)
    h = _submit(eng, b, qlens=qlens)
    assert eng.kernel_name() == LONG
    eng.sync()
    outc, idx = _traced(h)
    bad = np.flatnonzero(outc != exp)
    assert bad.size == 0, (bad[:8], outc[bad[:8]], exp[bad[:8]], qlens[bad[:8]])
    matched = exp == parity.CODE["matched"]
    di, cnt = np.unique(idx[matched], return_counts=True)
    assert parity.decode_rows(plan, dict(zip(di.tolist(), cnt.tolist())), False) == o.rows()
    _check_totals(eng, o.counters, o.rows(), n)
    eng.close()


def test_wave_per_read_kernel_wrapping_quality_bytes(generic):
    """quality bytes below '!' score 223..255 (`ch as u8 - 33` wraps, parse.rs:326)"""
    c = sc.small("plain")
    plan = _plan(c)
    w = cases.with_wrapping_quality(dict(c, reads=list(c["batches"]["P4"]["reads"])), seed=3)
    b = sc.make_batch(w["reads"], stride=336, use_lens=True)
    assert any(ord(ch) < 33 for _, q in w["reads"] for ch in q)
    eng = _engine(plan)
    h = _submit(eng, b)
    assert eng.kernel_name() == LONG
    eng.sync()
    o = _check_reads(c, plan, h, w["reads"])
    assert o.counters["low_quality"] > 0 and o.counters["matched"] > 0
    _check_totals(eng, o.counters, o.rows(), len(w["reads"]))
    eng.close()
